// rhj_block.h — the block of one chunk of a batched entry point: typed pieces in declaration order in a pinned host block,
// [read-back pieces: pinned only][uploaded pieces: mirrored at the same offset in a device buffer].  A piece begins on a
// multiple of its element's alignment (bases and the first uploaded piece on 8 bytes), and nothing else is padded.  The same
// declarations run twice: on a Block without bases for the sizes, then on one with them for the pointers.  No HIP in here.
#pragma once
#include <stddef.h>
#include <stdint.h>

class Block {
    static constexpr size_t NONE = ~(size_t)0;
    size_t at = 0, up_at = NONE;                                       // bytes declared; where the uploaded part begins
    uintptr_t pin, dev;                                                // the two bases; 0: this Block only sizes

    template <class T> size_t place(size_t count, size_t align)
    {
        static_assert(alignof(T) <= 8, "the bases of a block are aligned to 8 bytes only");
        const size_t off = at = (at + align - 1) / align * align;
        at += count * sizeof(T);
        return off;
    }

public:
    explicit Block(void *pinned = nullptr, void *device = nullptr) : pin((uintptr_t)pinned), dev((uintptr_t)device) {}
    template <class T> void back(T *&host, size_t count) { host = (T *)(pin + place<T>(count, alignof(T))); }     // in front of every up()
    template <class T> void up(T *&host, T *&device, size_t count)
    {
        const size_t off = place<T>(count, up_at == NONE ? 8 : alignof(T));
        if (up_at == NONE) up_at = off;
        host = (T *)(pin + off); device = (T *)(dev + (off - up_at));
    }
    size_t bytes() const { return at; }                                // of the pinned block
    size_t up_bytes() const { return up_at == NONE ? 0 : at - up_at; } // of its uploaded part: what the device buffer holds
    // a run of consecutive uploaded pieces is [first piece's host pointer, next piece's or host_end()): where the device has it
    char *host_end() const { return (char *)(pin + at); }
    void *mirror(const void *host) const { return (void *)(dev + ((uintptr_t)host - (pin + up_at))); }
};
