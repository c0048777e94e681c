/* ssw_top5_select.inc -- the selection network of the matrix-core top-N scan (K1a): the five
 * largest of a lane's keys, found from sorted TRIPLES of keys instead of key by key.
 * Part of the single translation unit ssw_kernels.hip (included there before ssw_k1a_mfma.inc);
 * tests/harness/top5_select_host.cpp compiles the same text for the host, with the three-input
 * operations below mapped to plain C. */
/*
 * Inserting a key into a sorted list of 5 costs 5 instructions (4 v_med3_f32 + v_max_f32), and a
 * key that cannot be among the final five pays them all the same: a wave cannot skip it lane by
 * lane.  Three instructions order three keys (v_max3 / v_med3 / v_min3), and then each RANK only
 * needs a list as long as that rank can ever fill:
 *
 *   Claim.  Cut a lane's keys into groups of three; call a group's largest r1, its middle r2 and
 *   its smallest r3.  The five largest keys S lie in
 *       (the 5 largest r1)  u  (the 2 largest r2)  u  (the largest r3).
 *   Proof.  A lane's keys are distinct (their low 7 bits are distinct labels), and a key outside
 *   S is below every key of S.  So the r1 in S are the largest r1, at most 5.  An r2 in S has its
 *   r1 in S: at most two such pairs fit, and their r2 are the largest r2.  An r3 in S has its
 *   whole group in S: one group at most, and its r3 is the largest r3.
 *
 * State: H[5], the list kept before; M[2], the two best r2; Z, the best r3.  A tile's 16 keys are
 * five triples and one leftover key that goes into H directly: 15 + 25 + 10 + 3 + 5 = 58 where 16
 * inserts were 80 (both beside the 16 labelling instructions).  M and Z are folded into H (15)
 * once per column block, before the halves of the wave swap lists; H is then what it always was,
 * key for key -- the 5th included, which the proof uses as its bound.
 *
 * The asm forms do not canonicalise their inputs (fmaxf would add a v_max per operand).  The
 * claim is about numbers.  With a NaN in a triple v_med3_f32 and v_min3_f32 both return the
 * smaller of the other two keys, which then enters M and Z alike and can sit in H twice after
 * the fold.  The scan never uses such lists: a NaN key (a feature beyond the binary16 range
 * makes every key of the frame -inf or NaN, and -inf with a label is a NaN; a NaN feature makes
 * the exact values NaN) comes with `am5 <= SSW_MFMA_XMAX` false or a failed strict order of the
 * four exact values in ptm_topn_mfma_kernel, so the frame is unproven, its floor is INT_MIN and
 * the exact pass rewrites it.  Whoever changes those two guards changes what this network may
 * be given.
 */
#ifndef SSW_SEL_FN
#define SSW_SEL_FN __device__ __forceinline__
SSW_SEL_FN float
ssw_sel_max2(float a, float b)
{
    float d;
    asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
SSW_SEL_FN float
ssw_sel_max3(float a, float b, float c)
{
    float d;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
SSW_SEL_FN float
ssw_sel_min3(float a, float b, float c)
{
    float d;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
SSW_SEL_FN float
ssw_sel_med3(float a, float b, float c)
{
    return __builtin_amdgcn_fmed3f(a, b, c);
}
#endif

/* one key into the sorted list of five (largest first) */
SSW_SEL_FN void
ssw_top5_insert(float (&H)[5], float key)
{
    H[4] = ssw_sel_med3(H[3], H[4], key);
    H[3] = ssw_sel_med3(H[2], H[3], key);
    H[2] = ssw_sel_med3(H[1], H[2], key);
    H[1] = ssw_sel_med3(H[0], H[1], key);
    H[0] = ssw_sel_max2(H[0], key);
}

SSW_SEL_FN void
ssw_top5_reset(float (&H)[5], float (&M)[2], float &Z, float neg_inf)
{
#pragma unroll
    for (int k = 0; k < 5; ++k)
        H[k] = neg_inf;
    M[0] = M[1] = Z = neg_inf;
}

/* the 16 labelled keys of one tile: five triples and the leftover 16th */
SSW_SEL_FN void
ssw_top5_tile(float (&H)[5], float (&M)[2], float &Z, const float (&key)[16])
{
    float r3_held = 0.0f;
#pragma unroll
    for (int g = 0; g < 5; ++g) {
        const float a = key[3 * g], b = key[3 * g + 1], c = key[3 * g + 2];
        const float r1 = ssw_sel_max3(a, b, c);
        const float r2 = ssw_sel_med3(a, b, c);
        const float r3 = ssw_sel_min3(a, b, c);
        ssw_top5_insert(H, r1);
        M[1] = ssw_sel_med3(M[0], M[1], r2);
        M[0] = ssw_sel_max2(M[0], r2);
        if (g & 1)
            Z = ssw_sel_max3(Z, r3_held, r3);
        else if (g == 4)
            Z = ssw_sel_max2(Z, r3);
        else
            r3_held = r3;
    }
    ssw_top5_insert(H, key[15]);
}

/* M and Z into H: from here on H is the list a key-by-key scan would have kept */
SSW_SEL_FN void
ssw_top5_fold(float (&H)[5], const float (&M)[2], float Z)
{
    ssw_top5_insert(H, M[0]);
    ssw_top5_insert(H, M[1]);
    ssw_top5_insert(H, Z);
}
