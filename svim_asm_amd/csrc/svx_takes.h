// svx_takes.h — the scratch of one call as ONE list: its size and its pointers come from the same slots.
// Host only and free of HIP, so that a plain C++ program can check it (tests/native/takes_sanitize.cpp).
//
// add() notes a pointer variable, an element size and a count; bytes() is what to reserve for the list; place() hands every
// slot its 256-aligned address, in list order.  A callee that needs scratch of its own takes the list by reference and adds
// to it before the caller lays it out (svx_stage_lay / svx_ws_lay in svx_internal.h).
#pragma once
#include <assert.h>
#include <stddef.h>
#include <string.h>
#include <type_traits>

static inline size_t svx_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct svx_takes {
    enum { kMax = 40 };
    struct slot {
        void* at;         // address of the caller's T* (null: the slot is only measured)
        size_t count, elem;
        const void* src;  // host source of an upload (add_up), else null
    };
    slot s[kMax];
    int n = 0;

    template <typename T>
    void add(T** at, size_t count) {
        assert(n < kMax);
        s[n++] = slot{(void*)at, count, sizeof(T), nullptr};
    }
    // as add(); the stage's lay-out also copies `count` elements from `src` to the slot (null src or no element: no copy)
    template <typename T, typename S>
    void add_up(T** at, const S* src, size_t count) {
        static_assert(std::is_same<typename std::remove_const<T>::type, S>::value, "the source has the slot's element type");
        add(at, count);
        s[n - 1].src = src;
    }
    size_t up_bytes(int i) const { return s[i].src ? s[i].count * s[i].elem : 0; }

    // every slot rounded up to 256 bytes plus the most its alignment can skip
    size_t bytes() const {
        size_t total = 0;
        for (int i = 0; i < n; ++i) total += svx_align_up(s[i].count * s[i].elem, 256) + 256;
        return total;
    }
    // slots from `base + used` on; returns the new `used` (at most the old one plus bytes())
    size_t place(char* base, size_t used) const {
        for (int i = 0; i < n; ++i) {
            const size_t off = svx_align_up(used, 256);
            used = off + s[i].count * s[i].elem;
            char* p = base + off;
            if (s[i].at) memcpy(s[i].at, &p, sizeof p);  // (the variable is a T*: written as the pointer it is)
        }
        return used;
    }
};
