// lane_harvest.cuh — mg_harvest_select / mg_harvest_download: the finished lanes of
// a batch chosen where the statuses are, and their rows gathered through a lane
// list (include/mythgpu.h states the contract).
//
// The selection is lane_rank.cuh's ranked selection for one class (the block geometry,
// the order and the skip list's invariant are stated there), after k_lane_mark on skipm:
//   k_harvest_scan    a lane matches when its status is below 32, that bit of the mask
//                     is set and it is not marked.
//   k_harvest_totals  one block.  The block offsets; n and matched; the eight maxima
//                     zeroed for the emit kernel.
//   k_harvest_emit    one thread per lane.  A matching lane of global rank r < max_lanes
//                     is selected: list[r] = lane.  The maxima of the eight counts are
//                     taken over the selected lanes only: a wave reduction, then at most
//                     one atomicMax per wave and field.
//
// None of the kernels writes the lane image.
//
// The gather kernels are mythgpu.hip's k_xfer_gather with the device lane taken
// from the list.  Invariant they rely on: every entry list[0 .. n) was written by
// k_harvest_emit from a thread whose lane index it is, so it is below n_lanes; the
// host never passes a count above the n that k_harvest_totals reported, and the
// list lives as long as the planes it indexes (mg_lanes_alloc, mg_sym_alloc and
// mg_explore_alloc drop the selection).
//
// mg_harvest_upload is the way back: k_xfer_place (below) and mythgpu.hip's
// k_xfer_scatter_idx write the listed lanes from the stage.  Their list is the resident
// one or the caller's, which the host checked with check_lane_list before any launch.
#pragma once

#define HV_NONE 0xffffffffu     // rank of a lane that does not match
#define HV_FIELDS 8u            // sp, msize, storage_count, trace_len, rec_len, n_nodes, n_consts, path_len

struct DevHarvest {
    uint32_t *skipm;    // [N] 1: the lane is in the call's skip list
    uint32_t *skip;     // [N] the call's skip list
    uint32_t *rank;     // [N] block-local rank among the matching lanes, or HV_NONE
    uint32_t *list;     // [N] the selection, ascending
    uint32_t *bt;       // [RK_MAX_BLOCKS] block totals
    uint32_t *boff;     // [RK_MAX_BLOCKS] exclusive block offsets
    uint32_t *info;     // [2 + HV_FIELDS] n, matched, the maxima (mg_harvest_info's first words)
};

// the per-lane counts the maxima are taken of; a null pointer is an absent plane
struct HarvestCounts {
    const uint32_t *f[HV_FIELDS];
};

__global__ __launch_bounds__(256) void k_harvest_scan(DevHarvest H, const uint32_t *__restrict__ status, uint32_t n,
                                                      uint32_t mask, uint32_t chunk) {
    const uint32_t lo = blockIdx.x * chunk;
    uint32_t carry = 0u;                                     // the block's carry over its tiles
    for (uint32_t t = 0; t < chunk; t += 256u) {
        const uint32_t l = lo + t + threadIdx.x;
        bool match[1] = {false};
        if (l < n) {
            const uint32_t st = status[l];
            match[0] = st < 32u && (mask >> st & 1u) && !H.skipm[l];
        }
        uint32_t r[1], tot[1];
        rank_tile<1>(match, r, tot);
        if (l < n) H.rank[l] = match[0] ? carry + r[0] : HV_NONE;
        carry += tot[0];
    }
    if (threadIdx.x == 0u) H.bt[blockIdx.x] = carry;
}

// one block of RK_MAX_BLOCKS threads: nb <= RK_MAX_BLOCKS block totals
__global__ __launch_bounds__(1024) void k_harvest_totals(DevHarvest H, uint32_t nb, uint32_t max_lanes) {
    const uint32_t t = threadIdx.x;
    const uint32_t v[1] = {t < nb ? H.bt[t] : 0u};
    uint32_t off[1], matched[1];
    rank_block_offsets<1>(v, off, matched);
    if (t < nb) H.boff[t] = off[0];
    if (t == 0u) { H.info[0] = min(matched[0], max_lanes); H.info[1] = matched[0]; }
    if (t < HV_FIELDS) H.info[2u + t] = 0u;
}

__global__ __launch_bounds__(256) void k_harvest_emit(DevHarvest H, HarvestCounts C, uint32_t n, uint32_t chunk,
                                                      uint32_t max_lanes) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    bool sel = false;
    if (l < n) {
        const uint32_t r = H.rank[l];
        if (r != HV_NONE) {
            const uint32_t g = H.boff[l / chunk] + r;        // <= l: the lanes below l that match
            if (g < max_lanes) { H.list[g] = l; sel = true; }
        }
    }
    if (!__ballot(sel)) return;                              // wave-uniform: nothing selected here
#pragma unroll
    for (uint32_t k = 0; k < HV_FIELDS; ++k) {
        uint32_t v = sel && C.f[k] ? C.f[k][l] : 0u;
#pragma unroll
        for (uint32_t d = 32u; d; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, (int)d, 64));
        if ((threadIdx.x & 63u) == 0u && v) atomicMax(&H.info[2u + k], v);
    }
}

// ---- indexed gathers: device lane list[l0 + l], not first + l0 + l ---------------
#define XP_MAX 24u
struct PickTable {              // the scalar fields of one download
    const void *src[XP_MAX];
    uint32_t off[XP_MAX];       // byte offset of the field in the stage
    uint32_t elem[XP_MAX];      // 4 or 8
};

// blockIdx.y = field; dst is 16-byte aligned and so is every off
__global__ __launch_bounds__(256) void k_xfer_pick(PickTable P, const uint32_t *__restrict__ list, uint32_t n,
                                                   uint8_t *__restrict__ dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (i >= n) return;
    const uint32_t lane = list[i];                           // < n_lanes (the invariant above)
    if (P.elem[f] == 8u) ((uint64_t *)(dst + P.off[f]))[i] = ((const uint64_t *)P.src[f])[lane];
    else ((uint32_t *)(dst + P.off[f]))[i] = ((const uint32_t *)P.src[f])[lane];
}

// ---- indexed placement (mg_harvest_upload): the inverse of k_xfer_pick ------------
// An entry with elem 4 or 8 copies stage element i to dst[list[i]]; an entry with elem 0
// is a fill: dst[list[i]] = off, a 4-byte constant (what the host does not supply
// starts clean, and a memset cannot follow a list).  At most XP_MAX copies and
// XP_FILL_MAX fills per launch.
#define XP_FILL_MAX 8u
struct PlaceTable {
    void *dst[XP_MAX + XP_FILL_MAX];
    uint32_t off[XP_MAX + XP_FILL_MAX];     // byte offset of the field in the stage; a fill's value
    uint32_t elem[XP_MAX + XP_FILL_MAX];    // 4 or 8; 0: a fill
};

// blockIdx.y = entry; src is 16-byte aligned and so is every off.  Every list entry is
// below n_lanes: the host checked it (check_lane_list) or k_harvest_emit wrote it.
__global__ __launch_bounds__(256) void k_xfer_place(PlaceTable P, const uint32_t *__restrict__ list, uint32_t n,
                                                    const uint8_t *__restrict__ src) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (i >= n) return;
    const uint32_t lane = list[i];
    if (P.elem[f] == 8u) ((uint64_t *)P.dst[f])[lane] = ((const uint64_t *)(src + P.off[f]))[i];
    else if (P.elem[f] == 4u) ((uint32_t *)P.dst[f])[lane] = ((const uint32_t *)(src + P.off[f]))[i];
    else ((uint32_t *)P.dst[f])[lane] = P.off[f];
}
