// svx_takes (svim_asm_amd/csrc/svx_takes.h) under AddressSanitizer + UBSan: a stand-alone program, the header alone.
// The arithmetic the list replaces is restated here in plain loops — align_up, a take that bumps `used`, take_bytes that a
// reserve summed — and every list is held to it: pointer for pointer, the final `used`, bytes(); the slots are 256-aligned
// and disjoint; a malloc of exactly bytes() is filled slot by slot, so a slot that reaches behind the sum is a report.
#include "svx_takes.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

static size_t r_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static size_t r_take_bytes(size_t count, size_t elem) { return r_align_up(count * elem, 256) + 256; }
static size_t r_take(size_t* used, size_t count, size_t elem) {  // the offset the take hands out
    const size_t off = r_align_up(*used, 256);
    *used = off + count * elem;
    return off;
}

struct E16 { uint64_t a, b; };
struct E24 { uint64_t a, b, c; };
static const size_t kElems[6] = {1, 2, 4, 8, 16, 24};

static int g_failed = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("line %d: %s does not hold\n", __LINE__, #cond);    \
            ++g_failed;                                                \
        }                                                              \
    } while (0)

// one slot of element size kElems[e] (its pointer: p[e]); src != 0: through add_up with that source
struct Ptrs {
    uint8_t* p1; uint16_t* p2; uint32_t* p4; uint64_t* p8; E16* p16; E24* p24;
    char* at(int e) const {
        switch (e) {
        case 0: return (char*)p1;
        case 1: return (char*)p2;
        case 2: return (char*)p4;
        case 3: return (char*)p8;
        case 4: return (char*)p16;
        default: return (char*)p24;
        }
    }
};
static void add_elem(svx_takes& t, Ptrs* p, int e, size_t count, bool null_slot) {
    switch (e) {
    case 0: t.add(null_slot ? (uint8_t**)nullptr : &p->p1, count); break;
    case 1: t.add(null_slot ? (uint16_t**)nullptr : &p->p2, count); break;
    case 2: t.add(null_slot ? (uint32_t**)nullptr : &p->p4, count); break;
    case 3: t.add(null_slot ? (uint64_t**)nullptr : &p->p8, count); break;
    case 4: t.add(null_slot ? (E16**)nullptr : &p->p16, count); break;
    default: t.add(null_slot ? (E24**)nullptr : &p->p24, count); break;
    }
}

// a list of one slot per element size with the given counts (counts[e]), placed at `used0` inside a malloc of exactly
// used0 + bytes() and filled; `null_mask`: slots added without a variable
static void placed_case(const size_t counts[6], size_t used0, unsigned null_mask) {
    svx_takes t;
    Ptrs p = {};
    for (int e = 0; e < 6; ++e) add_elem(t, &p, e, counts[e], (null_mask >> e) & 1u);
    size_t sum = 0, used = used0, off[6];
    for (int e = 0; e < 6; ++e) {
        sum += r_take_bytes(counts[e], kElems[e]);
        off[e] = r_take(&used, counts[e], kElems[e]);
    }
    EXPECT(t.bytes() == sum);
    // (the regions are 256-aligned in HBM; here the block is, so that "256-aligned" can be asked of the pointers)
    char* base = (char*)aligned_alloc(256, r_align_up(used0 + t.bytes(), 256));
    const size_t end = t.place(base, used0);
    EXPECT(end == used);
    EXPECT(end <= used0 + t.bytes());
    size_t prev_end = used0;
    for (int e = 0; e < 6; ++e) {
        if ((null_mask >> e) & 1u) {
            EXPECT(p.at(e) == nullptr);
        } else {
            EXPECT(p.at(e) == base + off[e]);
            EXPECT(((uintptr_t)p.at(e) & 255u) == 0);
        }
        EXPECT(off[e] >= prev_end);  // disjoint, in list order
        prev_end = off[e] + counts[e] * kElems[e];
    }
    free(base);
    // the fill: a block of EXACTLY used0 + bytes() bytes (malloc: its end is where the sanitizer watches)
    char* exact = (char*)malloc(used0 + t.bytes() ? used0 + t.bytes() : 1);
    t.place(exact, used0);
    for (int e = 0; e < 6; ++e)
        if (!((null_mask >> e) & 1u))
            for (size_t i = 0; i < counts[e] * kElems[e]; ++i) p.at(e)[i] = (char)(e + 1);
    for (int e = 0; e < 6; ++e)  // nothing overwritten by a later slot
        if (!((null_mask >> e) & 1u))
            for (size_t i = 0; i < counts[e] * kElems[e]; ++i) EXPECT(p.at(e)[i] == (char)(e + 1));
    free(exact);
}

// a callee's share of a list
struct Callee { uint32_t* a; E24* b; };
static void callee_adds(svx_takes& t, Callee* c, size_t n) {
    t.add(&c->a, n);
    t.add(&c->b, n + 1);
}

int main() {
    const size_t kCounts[5] = {0, 1, 255, 256, 257};
    const size_t kUsed[3] = {0, 4096, 4096 + 77};
    int lists = 0;
    // every count at every element size, the counts rotated over the sizes; every starting `used`
    for (size_t u = 0; u < 3; ++u)
        for (int r = 0; r < 5; ++r) {
            size_t counts[6];
            for (int e = 0; e < 6; ++e) counts[e] = kCounts[(e + r) % 5];
            placed_case(counts, kUsed[u], 0);
            placed_case(counts, kUsed[u], 0x2Au);  // null slots among the others
            lists += 2;
        }
    for (int c = 0; c < 5; ++c) {  // one count at all sizes
        size_t counts[6] = {kCounts[c], kCounts[c], kCounts[c], kCounts[c], kCounts[c], kCounts[c]};
        placed_case(counts, 4096 + 77, 0);
        ++lists;
    }
    {  // the empty list
        svx_takes t;
        EXPECT(t.bytes() == 0);
        char byte;
        EXPECT(t.place(&byte, 0) == 0 && t.place(&byte, 4096 + 77) == 4096 + 77);
    }
    {  // measured only: 2^32 + 1 elements of every size, no variable
        svx_takes t;
        const size_t n = ((size_t)1 << 32) + 1;
        size_t sum = 0;
        for (int e = 0; e < 6; ++e) {
            add_elem(t, nullptr, e, n, true);
            sum += r_take_bytes(n, kElems[e]);
        }
        EXPECT(t.bytes() == sum && sum > 55 * n);
    }
    for (size_t u = 0; u < 3; ++u) {  // a list extended by a second function == the same slots added in one place
        const size_t n = 257;
        uint8_t *x1, *x2;
        Callee c1, c2;
        svx_takes one, two;
        one.add(&x1, 3);
        one.add(&c1.a, n);
        one.add(&c1.b, n + 1);
        two.add(&x2, 3);
        callee_adds(two, &c2, n);
        EXPECT(one.n == two.n && one.bytes() == two.bytes());
        char* base = (char*)malloc(kUsed[u] + one.bytes());
        EXPECT(one.place(base, kUsed[u]) == two.place(base, kUsed[u]));
        EXPECT(x1 == x2 && c1.a == c2.a && c1.b == c2.b);
        for (size_t i = 0; i <= n; ++i) c2.b[i] = E24{i, i, i};
        for (size_t i = 0; i < n; ++i) c2.a[i] = (uint32_t)i;
        EXPECT(c1.b[n].c == n && c1.a[n - 1] == n - 1);
        free(base);
    }
    {  // uploads: the byte count comes from the element type; a null source and a zero count mean no copy
        const uint64_t src[4] = {1, 2, 3, 4};
        uint64_t *a, *b, *c;
        const uint64_t* d;
        uint32_t* e;
        svx_takes t;
        t.add_up(&a, src, 4);
        t.add_up(&b, (const uint64_t*)nullptr, 4);
        t.add_up(&c, src, 0);
        t.add_up(&d, src, 3);  // (a slot of pointers to const)
        t.add(&e, 5);
        EXPECT(t.up_bytes(0) == 32 && t.s[0].src == src);
        EXPECT(t.up_bytes(1) == 0 && t.up_bytes(2) == 0 && t.up_bytes(3) == 24 && t.up_bytes(4) == 0);
        svx_takes plain;
        plain.add(&a, 4); plain.add(&b, 4); plain.add(&c, 0); plain.add(&d, 3); plain.add(&e, 5);
        EXPECT(plain.bytes() == t.bytes());
        char* base = (char*)malloc(t.bytes());
        EXPECT(t.place(base, 0) <= t.bytes());
        for (int i = 0; i < t.n; ++i)  // what svx_stage_lay does with the list, on the host
            if (t.up_bytes(i)) memcpy(*(void**)t.s[i].at, t.s[i].src, t.up_bytes(i));
        EXPECT(a[3] == 4 && d[2] == 3);
        free(base);
    }
    if (g_failed) {
        printf("takes_sanitize: %d checks failed\n", g_failed);
        return 1;
    }
    printf("takes_sanitize ok: %d lists placed and filled\n", lists);
    return 0;
}
