// lane_explore.cuh — mg_explore: the plan of a fork round made on the device, and
// the per-lane record of the path a lane took (include/mythgpu.h states the
// contract; svm.py:293-337, jumpi_ instructions.py:1558-1636).
//
// A round is: step (launch_step), plan (the three kernels below), one readback of
// ExploreCtr, then lane_fork.cuh's k_fork_copy and k_fork_commit unmodified, then
// k_explore_path.  The plan fills the arrays of a ForkArgs in device memory; the
// host passes only counts by value.
//
//   k_explore_scan   one thread per lane.  fork_probe (lane_fork.cuh) classifies the
//                    lane; the forkable lanes are ranked in ascending lane order,
//                    separately for EX_INPLACE (invalid target: fall-through only)
//                    and EX_JUMP (needs a free lane): a __ballot / popcount rank
//                    inside each wave64, the four wave totals of a block through
//                    LDS, a running carry over the block's tiles.  Block b owns the
//                    lanes [b * chunk, (b + 1) * chunk), chunk a multiple of 256, so
//                    there are at most EX_MAX_BLOCKS block totals whatever n is.
//   k_explore_totals one block.  Exclusive scan of the block totals; the counters.
//   k_explore_emit   one thread per lane.  With K1 / K2 the lane's global ranks among
//                    the EX_INPLACE / EX_JUMP lanes and `avail` free lanes unused,
//                    an EX_JUMP lane forks when K2 < avail (the lowest lanes win) and
//                    is fork number K1 + min(K2, avail); its jump child is
//                    free[base + K2] and its copy is copy number K2.  Sources and the
//                    free list both ascend, so the copy list ascends by destination,
//                    which k_fork_copy's mapping relies on.
//
// No block waits for another: the three kernels are ordered by the stream.
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

#define EX_MAX_BLOCKS 1024u
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
    uint32_t *bt;         // [EX_MAX_BLOCKS][4] block totals: in place, jump, running, path full
    uint32_t *boff;       // [EX_MAX_BLOCKS][2] exclusive block offsets: in place, jump
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

__global__ __launch_bounds__(256) void k_explore_mark(DevExplore E, uint32_t n_free) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_free) E.isfree[E.free[j]] = 1u;   // the host checked every entry against n_lanes
}

__global__ __launch_bounds__(256) void k_explore_scan(DevLanes L, DevSym S, DevExplore E,
                                                      const DevCode *__restrict__ codes,
                                                      const uint8_t *__restrict__ a8,
                                                      const uint32_t *__restrict__ a32, uint32_t n_codes,
                                                      uint32_t chunk) {
    __shared__ uint32_t sh[4][4];
    const uint32_t x = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << x) - 1ull;
    const uint32_t lo = blockIdx.x * chunk;
    uint32_t c1 = 0u, c2 = 0u, c_run = 0u, c_full = 0u;      // the block's carry over its tiles
    for (uint32_t t = 0; t < chunk; t += 256u) {
        const uint32_t l = lo + t + threadIdx.x;
        uint32_t kind = EX_NONE, cond = 0u, jidx = MG_JRES_NONE;
        bool running = false;
        if (l < L.n) {
            running = L.status[l] == MG_RUNNING;
            if (!E.isfree[l] && fork_probe(L, S, codes, a8, a32, n_codes, l, true, cond, jidx))
                kind = E.path_len[l] >= E.path_cap ? EX_FULL : jidx != MG_JRES_NONE ? EX_JUMP : EX_INPLACE;
        }
        const unsigned long long b1 = __ballot(kind == EX_INPLACE), b2 = __ballot(kind == EX_JUMP);
        const unsigned long long br = __ballot(running), bf = __ballot(kind == EX_FULL);
        if (x == 0u) {
            sh[w][0] = (uint32_t)__popcll(b1); sh[w][1] = (uint32_t)__popcll(b2);
            sh[w][2] = (uint32_t)__popcll(br); sh[w][3] = (uint32_t)__popcll(bf);
        }
        __syncthreads();
        uint32_t p1 = 0u, p2 = 0u, t1 = 0u, t2 = 0u, tr = 0u, tf = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if (k < w) { p1 += sh[k][0]; p2 += sh[k][1]; }
            t1 += sh[k][0]; t2 += sh[k][1]; tr += sh[k][2]; tf += sh[k][3];
        }
        if (l < L.n) {
            E.kind[l] = kind;
            E.r1[l] = c1 + p1 + (uint32_t)__popcll(b1 & below);
            E.r2[l] = c2 + p2 + (uint32_t)__popcll(b2 & below);
            E.lcond[l] = cond; E.ljidx[l] = jidx;
        }
        c1 += t1; c2 += t2; c_run += tr; c_full += tf;
        __syncthreads();                                     // sh is rewritten by the next tile
    }
    if (threadIdx.x == 0u) {
        uint32_t *o = E.bt + 4u * blockIdx.x;
        o[0] = c1; o[1] = c2; o[2] = c_run; o[3] = c_full;
    }
}

// one block of EX_MAX_BLOCKS threads: nb <= EX_MAX_BLOCKS block totals
__global__ __launch_bounds__(1024) void k_explore_totals(DevExplore E, uint32_t nb, uint32_t avail,
                                                         const DevCounters *__restrict__ step_ctr, uint32_t n_step_ctr,
                                                         ExploreCtr *__restrict__ out) {
    __shared__ uint32_t s1[2][EX_MAX_BLOCKS], s2[2][EX_MAX_BLOCKS];
    __shared__ uint32_t s_run, s_full;
    __shared__ unsigned long long s_steps;
    const uint32_t t = threadIdx.x;
    if (t == 0u) { s_run = 0u; s_full = 0u; s_steps = 0ull; }
    const uint32_t v1 = t < nb ? E.bt[4u * t] : 0u, v2 = t < nb ? E.bt[4u * t + 1u] : 0u;
    s1[0][t] = v1; s2[0][t] = v2;
    __syncthreads();
    if (t < nb) { atomicAdd(&s_run, E.bt[4u * t + 2u]); atomicAdd(&s_full, E.bt[4u * t + 3u]); }
    unsigned long long steps = 0ull;
    for (uint32_t k = t; k < n_step_ctr; k += EX_MAX_BLOCKS) steps += step_ctr[k].lane_steps;
    if (steps) atomicAdd(&s_steps, steps);
    uint32_t cur = 0u;
    for (uint32_t d = 1u; d < EX_MAX_BLOCKS; d <<= 1) {      // inclusive scan, double-buffered
        const uint32_t a = s1[cur][t] + (t >= d ? s1[cur][t - d] : 0u);
        const uint32_t b = s2[cur][t] + (t >= d ? s2[cur][t - d] : 0u);
        s1[cur ^ 1u][t] = a; s2[cur ^ 1u][t] = b;
        cur ^= 1u;
        __syncthreads();
    }
    if (t < nb) { E.boff[2u * t] = s1[cur][t] - v1; E.boff[2u * t + 1u] = s2[cur][t] - v2; }
    if (t == 0u) {
        const uint32_t k1 = s1[cur][EX_MAX_BLOCKS - 1u], k2 = s2[cur][EX_MAX_BLOCKS - 1u];
        const uint32_t copies = min(k2, avail);
        out->forks = k1 + copies; out->copies = copies; out->running = s_run; out->starved = k2 - copies;
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
