// lane_explore.cuh — mg_explore: the plan of a fork round made on the device, and
// the per-lane record of the path a lane took (include/mythgpu.h states the
// contract; svm.py:293-337, jumpi_ instructions.py:1558-1636).
//
// A round is: step (launch_step), plan (the three kernels below), one readback of
// ExploreCtr, then lane_fork.cuh's k_fork_copy and k_fork_commit unmodified, then
// k_explore_path.  The plan fills the arrays of a ForkArgs in device memory; the
// host passes only counts by value.
//
// The plan is lane_rank.cuh's ranked selection (the block geometry, the order and the
// free list's invariant are stated there), after k_lane_mark on isfree:
//   k_explore_scan   fork_probe (lane_fork.cuh) classifies the lane.  Ranked: EX_INPLACE
//                    (invalid target: fall-through only) and EX_JUMP (needs a free
//                    lane); only counted: the running and the path-full lanes.
//   k_explore_totals one block.  Offsets of the two ranked classes; the counters.
//   k_explore_emit   one thread per lane.  With K1 / K2 the lane's global ranks among
//                    the EX_INPLACE / EX_JUMP lanes and `avail` free lanes unused,
//                    an EX_JUMP lane forks when K2 < avail (the lowest lanes win) and
//                    is fork number K1 + min(K2, avail); its jump child is
//                    free[base + K2] and its copy is copy number K2.  Sources and the
//                    free list both ascend, so the copy list ascends by destination,
//                    which k_fork_copy's mapping relies on.
//
// Read-before-write: the fall-through is in place (dst_fall == src), so the jump
// child is copied from a lane the fall-through update rewrites.  Nothing before
// k_fork_commit writes a source lane: a lane marked free is never a source
// (k_explore_scan skips it; the mark is cleared only when the lane is handed out),
// the free list is strictly ascending, so sources and destinations are all
// distinct; k_fork_copy reads unmodified sources; k_fork_commit runs after it on
// the same stream and its thread reads its source before it writes anything.
// k_explore_path runs after that and touches only the path planes: its thread
// reads the source's path_len, root and rows, writes them to the jump child (another
// lane), and only then appends to the source; the appended entry lies at path_len,
// above every row it read, and no other thread touches that fork's lanes.
#pragma once

#define EX_NONE 0u      // not a source
#define EX_INPLACE 1u   // forkable, the target is no JUMPDEST: fall-through only, no free lane
#define EX_JUMP 2u      // forkable with a valid target: needs one free lane
#define EX_FULL 3u      // forkable but path_len == path_cap: left as it is

struct DevExplore {
    uint32_t path_cap;
    uint32_t *path;       // [path_cap][N]  cond_tag << 1 | side
    uint32_t *path_len;   // [N]
    uint32_t *root;       // [N]
    // plan scratch, [N] each
    uint32_t *isfree;     // 1: the lane is in the unused part of the free list
    uint32_t *free;       // the call's free list
    uint32_t *kind, *r1, *r2, *lcond, *ljidx;   // per lane: class, block-local ranks, probe results
    uint32_t *bt;         // [RK_MAX_BLOCKS][4] block totals: in place, jump, running, path full
    uint32_t *boff;       // [RK_MAX_BLOCKS][2] exclusive block offsets: in place, jump
    uint32_t *fork;       // [8][N] the ForkArgs arrays: src, dst_fall, dst_jump, copy_fork, copy_dst, made, cond, jidx
};

struct ExploreCtr {
    uint32_t forks, copies, running, starved, path_full, _pad;
    unsigned long long lane_steps;
};

__global__ __launch_bounds__(256) void k_explore_init(DevExplore E, uint32_t n) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n) return;
    E.root[l] = l; E.path_len[l] = 0u; E.isfree[l] = 0u;
}

__global__ __launch_bounds__(256) void k_explore_scan(DevLanes L, DevSym S, DevExplore E,
                                                      const DevCode *__restrict__ codes, const uint8_t *__restrict__ a8,
                                                      const uint32_t *__restrict__ a32, uint32_t n_codes, uint32_t chunk) {
    const uint32_t lo = blockIdx.x * chunk;
    uint32_t c[4] = {0u, 0u, 0u, 0u};                        // the block's carries over its tiles
    for (uint32_t t = 0; t < chunk; t += 256u) {
        const uint32_t l = lo + t + threadIdx.x;
        uint32_t kind = EX_NONE, cond = 0u, jidx = MG_JRES_NONE;
        bool running = false;
        if (l < L.n) {
            running = L.status[l] == MG_RUNNING;
            if (!E.isfree[l] && fork_probe(L, S, codes, a8, a32, n_codes, l, true, cond, jidx))
                kind = E.path_len[l] >= E.path_cap ? EX_FULL : jidx != MG_JRES_NONE ? EX_JUMP : EX_INPLACE;
        }
        const bool flag[4] = {kind == EX_INPLACE, kind == EX_JUMP, running, kind == EX_FULL};
        uint32_t r[4], tot[4];                               // r[2] and r[3] are not read
        rank_tile<4>(flag, r, tot);
        if (l < L.n) {
            E.kind[l] = kind;
            E.r1[l] = c[0] + r[0]; E.r2[l] = c[1] + r[1];
            E.lcond[l] = cond; E.ljidx[l] = jidx;
        }
        c[0] += tot[0]; c[1] += tot[1]; c[2] += tot[2]; c[3] += tot[3];
    }
    if (threadIdx.x == 0u) {
        uint32_t *o = E.bt + 4u * blockIdx.x;                // in place, jump, running, path full
        o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[3];
    }
}

// one block of RK_MAX_BLOCKS threads: nb <= RK_MAX_BLOCKS block totals
__global__ __launch_bounds__(1024) void k_explore_totals(DevExplore E, uint32_t nb, uint32_t avail,
                                                         const DevCounters *__restrict__ step_ctr, uint32_t n_step_ctr,
                                                         ExploreCtr *__restrict__ out) {
    __shared__ uint32_t s_run, s_full;
    __shared__ unsigned long long s_steps;
    const uint32_t t = threadIdx.x;
    if (t == 0u) { s_run = 0u; s_full = 0u; s_steps = 0ull; }
    const uint32_t v[2] = {t < nb ? E.bt[4u * t] : 0u, t < nb ? E.bt[4u * t + 1u] : 0u};
    __syncthreads();
    if (t < nb) { atomicAdd(&s_run, E.bt[4u * t + 2u]); atomicAdd(&s_full, E.bt[4u * t + 3u]); }
    unsigned long long steps = 0ull;
    for (uint32_t i = t; i < n_step_ctr; i += RK_MAX_BLOCKS) steps += step_ctr[i].lane_steps;
    if (steps) atomicAdd(&s_steps, steps);
    uint32_t off[2], k[2];
    rank_block_offsets<2>(v, off, k);                        // its barriers order the three sums too
    if (t < nb) { E.boff[2u * t] = off[0]; E.boff[2u * t + 1u] = off[1]; }
    if (t == 0u) {
        const uint32_t copies = min(k[1], avail);
        out->forks = k[0] + copies; out->copies = copies; out->running = s_run; out->starved = k[1] - copies;
        out->path_full = s_full; out->_pad = 0u; out->lane_steps = s_steps;
    }
}

__global__ __launch_bounds__(256) void k_explore_emit(DevExplore E, uint32_t n, uint32_t N, uint32_t chunk,
                                                      uint32_t base, uint32_t avail) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n) return;
    const uint32_t kind = E.kind[l];
    if (kind != EX_INPLACE && kind != EX_JUMP) return;
    const uint32_t b = l / chunk;
    const uint32_t k1 = E.boff[2u * b] + E.r1[l], k2 = E.boff[2u * b + 1u] + E.r2[l];
    if (kind == EX_JUMP && k2 >= avail) return;              // starved: wholly untouched
    const uint32_t f = k1 + min(k2, avail);                  // < n: one fork per lane at most
    uint32_t *src = E.fork, *dst_fall = src + N, *dst_jump = dst_fall + N, *copy_fork = dst_jump + N,
             *copy_dst = copy_fork + N, *made = copy_dst + N, *cond = made + N, *jidx = cond + N;
    src[f] = l; dst_fall[f] = l; cond[f] = E.lcond[l];
    if (kind == EX_JUMP) {
        const uint32_t d = E.free[base + k2];                // base + k2 < n_free
        dst_jump[f] = d; made[f] = MG_FORK_MADE_FALL | MG_FORK_MADE_JUMP; jidx[f] = E.ljidx[l];
        copy_fork[k2] = f | FORK_COPY_JUMP; copy_dst[k2] = d;
        E.isfree[d] = 0u;
    } else {
        dst_jump[f] = MG_FORK_NONE; made[f] = MG_FORK_MADE_FALL; jidx[f] = MG_JRES_NONE;
    }
}

// one thread per fork, after k_fork_commit
__global__ __launch_bounds__(256) void k_explore_path(DevExplore E, uint32_t N, ForkArgs F) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F.n) return;
    const uint32_t s = F.src[i], m = F.made[i], tag = F.cond[i];
    const uint32_t len = E.path_len[s], root = E.root[s];    // the plan saw len < path_cap
    if (m & MG_FORK_MADE_JUMP) {
        const uint32_t d = F.dst_jump[i];
        for (uint32_t e = 0; e < len; ++e) E.path[(size_t)e * N + d] = E.path[(size_t)e * N + s];
        E.path[(size_t)len * N + d] = tag << 1 | 1u;
        E.path_len[d] = len + 1u; E.root[d] = root;
    }
    E.path[(size_t)len * N + s] = tag << 1;
    E.path_len[s] = len + 1u;
}
