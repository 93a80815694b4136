// lane_rank.cuh — ranked selection: the lanes of a class numbered in ascending lane
// order.  mg_explore's fork plan (lane_explore.cuh) and mg_harvest_select
// (lane_harvest.cuh) both use it; what they share is stated here, once.
//
//   mark    k_lane_mark sets marks[list[j]] in a cleared plane.  The host checked the
//           list (mythgpu.hip, check_lane_list): below n_lanes, strictly ascending.
//   scan    block b owns the lanes [b * chunk, (b + 1) * chunk), chunk a multiple of 256
//           (rank_geometry): at most RK_MAX_BLOCKS block totals whatever n is.  rank_tile
//           ranks a tile; the kernel stores carry + rank, its carry running over the tiles.
//   totals  one block: rank_block_offsets makes exclusive block offsets of the totals.
//   emit    offset[lane / chunk] + the stored rank: the lanes of the class below this one.
//
// No block waits for another: the kernels are ordered by the stream.
#pragma once

#define RK_MAX_BLOCKS 1024u

__global__ __launch_bounds__(256) void k_lane_mark(uint32_t *marks, const uint32_t *list, uint32_t n) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) marks[list[j]] = 1u;
}

// rank[k]: the threads below this one whose flag[k] is set; total[k]: those of the tile.
// A __ballot / popcount rank inside each wave64, the four wave totals through LDS.
// Contract: every thread of a 256-thread block calls it (it holds two __syncthreads()),
// the waves are wave64, the LDS scratch is free again when it returns.  An output the
// caller does not read compiles away.
template <uint32_t K>
__device__ __forceinline__ void rank_tile(const bool (&flag)[K], uint32_t (&rank)[K], uint32_t (&total)[K]) {
    __shared__ uint32_t sh[4][K];
    const uint32_t x = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << x) - 1ull;
    unsigned long long b[K];
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) { b[k] = __ballot(flag[k]); if (x == 0u) sh[w][k] = (uint32_t)__popcll(b[k]); }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {
        rank[k] = (uint32_t)__popcll(b[k] & below);
        total[k] = 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            if (j < w) rank[k] += sh[j][k];
            total[k] += sh[j][k];
        }
    }
    __syncthreads();                            // sh is rewritten by the next call
}

// v[k]: this thread's block total (0 past the last block).  excl[k]: the sum over the
// threads below; grand[k]: over all.  Contract: every thread of one block of RK_MAX_BLOCKS
// threads calls it; it synchronises after its stores and every pass, not after the last reads.
template <uint32_t K>
__device__ __forceinline__ void rank_block_offsets(const uint32_t (&v)[K], uint32_t (&excl)[K], uint32_t (&grand)[K]) {
    __shared__ uint32_t s[2][K][RK_MAX_BLOCKS];
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) s[0][k][t] = v[k];
    __syncthreads();
    uint32_t cur = 0u;
    for (uint32_t d = 1u; d < RK_MAX_BLOCKS; d <<= 1) {     // inclusive scan, double-buffered
#pragma unroll
        for (uint32_t k = 0; k < K; ++k) s[cur ^ 1u][k][t] = s[cur][k][t] + (t >= d ? s[cur][k][t - d] : 0u);
        cur ^= 1u;
        __syncthreads();
    }
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) { excl[k] = s[cur][k][t] - v[k]; grand[k] = s[cur][k][RK_MAX_BLOCKS - 1u]; }
}
