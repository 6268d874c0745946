// adfp_scan.h -- the integer scans of the mesh tools: the exclusive prefix over a workgroup, and the device-wide exclusive scan of
// a predicate over n items in three launches (used by the mesh clean-up, the voxel down-sample and, its middle kernel, the bound):
//
//   k_scan_count   a workgroup counts the set items of its tile of 256 x PER items          -> tile_counts[tile]
//   k_tile_scan    ONE workgroup: the exclusive prefix of the tile counts, LANES x PER tiles a round with the carry of the rounds
//                  before                                                                     -> tile_offsets[tile], total[0]
//   k_scan_place   the tile again: an item's position = its tile's offset + the set items before it in the tile
//
// Counts are integers, so no result depends on the shape of a launch.
#pragma once
#include "adfp_device.h"

#define ADFP_SCAN_THREADS 256          // workgroup of the count and place kernels

// exclusive prefix of v over the workgroup (NT threads, wave64); total = the sum over the workgroup.  lds: NT / 64 slots.
template <typename T, int NT>
ADFP_DEV T block_scan(T v, T& total, T* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const T s = lds[w];
        base += (w < wave) ? s : (T)0;
        tot += s;
    }
    __syncthreads();                                  // lds is reused by the next call
    total = tot;
    return base + x - v;
}

// the predicate of a byte-flag array (a PRED is any such functor: is item i set?)
struct FlagSet {
    const unsigned char* flag;
    ADFP_DEV bool operator()(long long i) const { return flag[i] != 0; }
};

template <int PER, typename PRED>
__global__ __launch_bounds__(ADFP_SCAN_THREADS) void k_scan_count(PRED pred, long long n, unsigned* __restrict__ tile_counts) {
    __shared__ unsigned lds[ADFP_SCAN_THREADS / 64];
    const long long first = ((long long)blockIdx.x * ADFP_SCAN_THREADS + threadIdx.x) * PER;
    unsigned c = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) c += (first + q < n && pred(first + q)) ? 1u : 0u;
    unsigned tot;
    block_scan<unsigned, ADFP_SCAN_THREADS>(c, tot, lds);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = tot;
}

// one workgroup: exclusive prefix of the tile counts, PER consecutive tiles per thread per round
template <int LANES, int PER>
__global__ __launch_bounds__(LANES) void k_tile_scan(const unsigned* __restrict__ tile_counts, long long ntiles, long long* __restrict__ tile_offsets,
                                                      long long* __restrict__ total) {
    __shared__ unsigned long long lds[LANES / 64];
    unsigned long long carry = 0;
    const long long per_round = (long long)LANES * PER;
    for (long long t0 = 0; t0 < ntiles; t0 += per_round) {
        const long long first = t0 + (long long)threadIdx.x * PER;
        unsigned cv[PER];
        unsigned long long s = 0;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            cv[q] = first + q < ntiles ? tile_counts[first + q] : 0u;
            s += cv[q];
        }
        unsigned long long tot;
        unsigned long long o = carry + block_scan<unsigned long long, LANES>(s, tot, lds);
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            if (first + q < ntiles) tile_offsets[first + q] = (long long)o;
            o += cv[q];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) total[0] = (long long)carry;
}

// STARTS false: out[i] = the number of set items before i, for every i < n.  STARTS true: out[k] = i for the k-th set item i.
template <int PER, bool STARTS, typename PRED>
__global__ __launch_bounds__(ADFP_SCAN_THREADS) void k_scan_place(PRED pred, long long n, const long long* __restrict__ tile_offsets,
                                                                   int* __restrict__ out) {
    __shared__ unsigned lds[ADFP_SCAN_THREADS / 64];
    const long long first = ((long long)blockIdx.x * ADFP_SCAN_THREADS + threadIdx.x) * PER;
    bool h[PER];
    unsigned c = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        h[q] = first + q < n && pred(first + q);
        c += h[q] ? 1u : 0u;
    }
    unsigned tot;
    long long p = tile_offsets[blockIdx.x] + block_scan<unsigned, ADFP_SCAN_THREADS>(c, tot, lds);
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        if (STARTS) { if (h[q]) out[p] = (int)(first + q); }
        else if (first + q < n) out[first + q] = (int)p;
        p += h[q] ? 1 : 0;
    }
}

// the three launches over n items: tc / to hold ceil(n / (256 PER)) entries each; total[0] = the number of set items
template <int PER, int SCAN_LANES, int SCAN_PER, bool STARTS, typename PRED>
static int scan_items(PRED pred, long long n, unsigned* tc, long long* to, int* out, long long* total, hipStream_t st) {
    if (n == 0) { hipError_t e = hipMemsetAsync(total, 0, sizeof(long long), st); return e == hipSuccess ? 0 : (int)e; }
    const long long ntiles = ceil_div(n, ADFP_SCAN_THREADS * PER);
    hipLaunchKernelGGL((k_scan_count<PER, PRED>), dim3((unsigned)ntiles), dim3(ADFP_SCAN_THREADS), 0, st, pred, n, tc);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_tile_scan<SCAN_LANES, SCAN_PER>), dim3(1), dim3(SCAN_LANES), 0, st, tc, ntiles, to, total);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_scan_place<PER, STARTS, PRED>), dim3((unsigned)ntiles), dim3(ADFP_SCAN_THREADS), 0, st, pred, n, to, out);
    ADFP_CHECK_LAUNCH();
    return 0;
}
