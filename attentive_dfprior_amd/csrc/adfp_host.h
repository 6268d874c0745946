// adfp_host.h -- host-only helpers of the launchers: rounding, block counts and the workspace arena.
//
// A tool's workspace layout is written ONCE, as a function that takes an Arena and the sizes, fills the tool's work struct with
// take<T>() in the buffers' order and returns it.  The size query runs that function on an arena without a base and returns
// bytes(); the launcher runs it on the caller's pointer.  What is measured is what is carved.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "adfp_sort.h"

static size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
static long long ceil_div(long long n, long long d) { return (n + d - 1) / d; }

static const long long RECON_MAX_N = 0x7fffffffll - ADFP_RS_TILE;       // the sort's tile arithmetic is int
// the radix sort's table for n pairs: [digits][tiles] counts + [digits] totals
static size_t sort_table_bytes(long long n) { return ((size_t)ceil_div(n, ADFP_RS_TILE) + 1) * ADFP_RS_DIGITS * 4; }

// (addresses are formed as integers: a size query carves a null base, and pointer arithmetic on NULL is undefined)
struct Arena {
    uintptr_t base; size_t off;
    explicit Arena(const void* p = nullptr) : base((uintptr_t)p), off(0) {}
    template <typename T> T* take(size_t count) { T* p = (T*)(base + off); off += al256(count * sizeof(T)); return p; }      // 256-byte blocks
    template <typename T> T* take_tail(size_t count) { T* p = (T*)(base + off); off += count * sizeof(T); return p; }        // a last block, not rounded
    size_t bytes() const { return off; }
};
// what a layout function takes from an arena: layout(arena, args...) measured without a base
template <typename F, typename... Args> static size_t layout_bytes(F layout, Args&&... args) { Arena A; layout(A, args...); return A.bytes(); }
