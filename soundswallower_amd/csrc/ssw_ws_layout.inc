/* ssw_ws_layout.inc -- host: the layout of one device workspace.  Plain C++17, no HIP header:
 * ssw_kernels.hip includes it ahead of the ssw_host_*.inc files, and a host program can include
 * it on its own (tests/harness/ws_layout_host.cpp). */
#include <cstddef>
#include <cstring>
#include <vector>

static inline size_t
align256(size_t x)
{
    return (x + 255) & ~(size_t)255;
}

/* Hands out offsets into one workspace in call order, every piece at a 256-byte boundary, and
 * remembers which pieces have a host source, so that "one staging buffer, one copy" is written
 * once: the caller keeps the offset each call returns (no piece has a number), fill() stages
 * the uploaded pieces, and a mark() names a boundary between them (what is cached on the device
 * and what a call uploads again).  A piece registered with the pointer that is to address it (the
 * typed overloads) is named once: resolve() sets every such pointer when the workspace is there. */
struct WsLayout {
    struct Piece {
        const void *src;
        size_t bytes, off;
    };
    struct Slot {
        void *ptr; /* a T * of the caller's: where resolve() writes the piece's address */
        size_t off;
    };
    std::vector<Piece> ins;
    std::vector<Slot> slots;
    size_t end = 0;    /* of the last piece, rounded up: where the next one goes */
    size_t in_end = 0; /* the same behind the last uploaded piece */

    WsLayout()
    {
        ins.reserve(32);
        slots.reserve(40);
    }
    /* an uploaded table; zero bytes take no space (the next piece then has the same offset).
     * `room` > bytes: the space it takes nevertheless */
    size_t in(const void *src, size_t bytes, size_t room = 0)
    {
        const size_t at = out(bytes > room ? bytes : room);
        ins.push_back(Piece{ src, bytes, at });
        in_end = end;
        return at;
    }
    /* device-only space */
    size_t out(size_t bytes)
    {
        const size_t at = end;
        end = align256(end + bytes);
        return at;
    }
    /* the same, and *slot = the piece's address once resolve() knows the workspace's (a piece of
     * zero bytes gets the address of whatever follows it) */
    template <typename T>
    size_t in(T **slot, const void *src, size_t bytes, size_t room = 0)
    {
        const size_t at = in(src, bytes, room);
        slots.push_back(Slot{ slot, at });
        return at;
    }
    template <typename T>
    size_t out(T **slot, size_t bytes)
    {
        const size_t at = out(bytes);
        slots.push_back(Slot{ slot, at });
        return at;
    }
    /* after devbuf_reserve: every registered pointer = base + its piece's offset (the pointer's
     * value is copied: a T ** is not a void **) */
    void resolve(unsigned char *base) const
    {
        for (const Slot &s : slots) {
            unsigned char *at = base + s.off;
            memcpy(s.ptr, &at, sizeof(at));
        }
    }
    size_t mark() const { return end; }
    size_t size() const { return end; }
    size_t in_bytes() const { return in_end; }
    /* every uploaded piece at or beyond `from`, to stage + (its offset - from): the caller then
     * copies [from, in_bytes()) in one piece.  Writes nothing but the pieces' own bytes. */
    void fill(unsigned char *stage, size_t from) const
    {
        for (const Piece &p : ins)
            if (p.bytes != 0 && p.off >= from)
                memcpy(stage + (p.off - from), p.src, p.bytes);
    }
};

/* the typed pointer of the piece at `off` in the workspace `ws` */
template <typename T>
static inline T *
ws_at(unsigned char *ws, size_t off)
{
    return reinterpret_cast<T *>(ws + off);
}
