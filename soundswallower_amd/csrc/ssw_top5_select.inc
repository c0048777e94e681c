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
 * Two levels (ssw_top5_tile2 / ssw_top5_fold2, what the scan runs).  Even so every r1 pays the
 * full insert, and the claim holds for the r1 as well as for the keys: a tile's five r1 and its
 * leftover 16th key are two more triples, (r1_0, r1_1, r1_2) and (r1_3, r1_4, key[15]), sorted
 * into s1 >= s2 >= s3; only s1 is inserted into H, s2 goes into a list of two, N, and the two s3
 * into Y with one v_max3.
 *
 *   Claim.  The five largest keys S lie in H u N u Y u M u Z.
 *   Proof.  A key above a member of S is in S.  An s2 in S has its s1 in S: such pairs are
 *   disjoint, at most two fit, so the s2 in S are the two largest s2.  An s3 in S has the s1 and
 *   the s2 of its triple in S, so it is the largest s3.  M and Z as before (an r2 in S has its r1
 *   in S, whichever list that r1 went to).  Y cannot share a register with Z: an s3 is the r1
 *   of a level-1 triple, and {s1, s2, s3 = r1, r2, r3} is a possible S with both in it.
 *
 * A tile is 15 + 6 + 10 + 4 + 1 + 10 + 3 = 49 instructions for 58.  The fold knows where a key
 * can land: ssw_top5_insert_from<FROM> is for a key below H[FROM - 1], touches the positions
 * FROM..4 only and costs 5 - FROM.  In fold order, with the keys above it that are in H by then
 * (or were pushed out of it by five larger ones):
 *   N[0]  1  its s1                       M[0]  1  its r1, or the s1 above that
 *   N[1]  3  its s1, N[0] and N[0]'s s1   M[1]  3  M[0] and the two r1 (the 3 largest of the r1
 *   Y     2  its s1, and its s2 or N[0]            and M[0] are in H: the claim, for three)
 *                                         Z     2  its r1 and r2 (the 2 largest of r1 u r2)
 * 18 instructions for six keys; a column block is 4 x 49 + 18 = 214 where it was 4 x 58 + 15 =
 * 247.  The same holds for the merge of two sorted lists (ssw_top5_merge): when the k-th entry of
 * the other list comes, k larger ones are in H already: 15 instructions for 25.
 *
 * The asm forms do not canonicalise their inputs (fmaxf would add a v_max per operand).  The
 * claim is about numbers.  With a NaN in a triple v_med3_f32 and v_min3_f32 both return the
 * smaller of the other two keys, which then enters M and Z alike and can sit in H twice after
 * the fold; with two levels the same happens one level up (a NaN r1 puts one key into N and Y
 * alike), and an insert that starts at FROM takes the list's order above FROM on trust, which a
 * NaN in the list breaks.  The scan never uses such lists: a NaN key (a feature beyond the binary16 range
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

/* a key below H[FROM - 1] into the sorted list: the positions FROM..4 only */
template <int FROM>
SSW_SEL_FN void
ssw_top5_insert_from(float (&H)[5], float key)
{
    static_assert(FROM >= 0 && FROM < 5, "a position of the list");
#pragma unroll
    for (int k = 4; k >= (FROM > 0 ? FROM : 1); --k)
        H[k] = ssw_sel_med3(H[k - 1], H[k], key);
    if (FROM == 0)
        H[0] = ssw_sel_max2(H[0], key);
}

/* the two-level network's state: N[2], the two best s2, and Y, the best s3, beside H, M and Z */
SSW_SEL_FN void
ssw_top5_reset2(float (&H)[5], float (&N)[2], float &Y, float (&M)[2], float &Z, float neg_inf)
{
    ssw_top5_reset(H, M, Z, neg_inf);
    N[0] = N[1] = Y = neg_inf;
}

/* the 16 labelled keys of one tile: five triples, then their r1 and the leftover 16th as two */
SSW_SEL_FN void
ssw_top5_tile2(float (&H)[5], float (&N)[2], float &Y, float (&M)[2], float &Z,
               const float (&key)[16])
{
    float r1[6], r3_held = 0.0f, s3_held = 0.0f;
#pragma unroll
    for (int g = 0; g < 5; ++g) {
        const float a = key[3 * g], b = key[3 * g + 1], c = key[3 * g + 2];
        r1[g] = ssw_sel_max3(a, b, c);
        const float r2 = ssw_sel_med3(a, b, c);
        const float r3 = ssw_sel_min3(a, b, c);
        M[1] = ssw_sel_med3(M[0], M[1], r2);
        M[0] = ssw_sel_max2(M[0], r2);
        if (g & 1)
            Z = ssw_sel_max3(Z, r3_held, r3);
        else if (g == 4)
            Z = ssw_sel_max2(Z, r3);
        else
            r3_held = r3;
    }
    r1[5] = key[15];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const float a = r1[3 * g], b = r1[3 * g + 1], c = r1[3 * g + 2];
        const float s1 = ssw_sel_max3(a, b, c);
        const float s2 = ssw_sel_med3(a, b, c);
        const float s3 = ssw_sel_min3(a, b, c);
        ssw_top5_insert(H, s1);
        N[1] = ssw_sel_med3(N[0], N[1], s2);
        N[0] = ssw_sel_max2(N[0], s2);
        if (g & 1)
            Y = ssw_sel_max3(Y, s3_held, s3);
        else
            s3_held = s3;
    }
}

/* N, Y, M and Z into H, each from the position it can reach (the table above): from here on H
 * is the list a key-by-key scan would have kept */
SSW_SEL_FN void
ssw_top5_fold2(float (&H)[5], const float (&N)[2], float Y, const float (&M)[2], float Z)
{
    ssw_top5_insert_from<1>(H, N[0]);
    ssw_top5_insert_from<3>(H, N[1]);
    ssw_top5_insert_from<2>(H, Y);
    ssw_top5_insert_from<1>(H, M[0]);
    ssw_top5_insert_from<3>(H, M[1]);
    ssw_top5_insert_from<2>(H, Z);
}

/* a second sorted list of five (no key in common with H) into H, by position */
SSW_SEL_FN void
ssw_top5_merge(float (&H)[5], const float (&G)[5])
{
    ssw_top5_insert_from<0>(H, G[0]);
    ssw_top5_insert_from<1>(H, G[1]);
    ssw_top5_insert_from<2>(H, G[2]);
    ssw_top5_insert_from<3>(H, G[3]);
    ssw_top5_insert_from<4>(H, G[4]);
}
