// lane_fork.cuh — mg_lanes_fork: the JUMPI fork of symbolic lanes as a lane-image
// operation (include/mythgpu.h states the contract; jumpi_, instructions.py:1558-1636).
//
// A fork copies the LIVE rows of a source lane into up to two free lanes of the
// lane-interleaved planes (device_state.h) and rewrites a handful of scalars.
// Three launches on the context's stream, whatever the number of forks:
//
//   k_fork_check   one thread per fork.  Reads the source's scalars, its top two
//                  tags and its target word; decides forkability and the jump's
//                  validity; writes made / cond / the resolved jump index.
//   k_fork_copy    the gather/scatter.  The host lists one copy per successor that
//                  lives in another lane than its source, SORTED BY DESTINATION LANE.
//                  Thread x of a wave takes copy (64 * blockIdx.x + x), so successors
//                  in neighbouring lanes are written by neighbouring threads: a plane
//                  row of 64 adjacent destinations is one contiguous run per store
//                  instruction (16 bytes per thread on the uint4 planes), and the two
//                  children of one parent read the same source address (one request).
//                  The rows of a copy are dealt round-robin to the grid's row workers
//                  (4 waves per block x gridDim.y), each bounded by the source's own
//                  live counts: nothing above them is read or written.
//   k_fork_commit  one thread per fork.  Reads every scalar of the source into
//                  registers, then writes the successors' scalars.
//
// Read-before-write: with dst_fall == src the jump child is copied from a lane the
// fall-through update rewrites.  Nothing before k_fork_commit writes a source lane
// (the host refuses a destination that is any fork's source, except the in-place
// fall-through, which needs no copy), so k_fork_check and k_fork_copy read
// unmodified sources; k_fork_commit runs after them on the same stream, its thread
// reads its source before it writes anything, and no other thread touches that
// fork's lanes (sources and destinations are all distinct).
#pragma once

typedef unsigned int v2u __attribute__((ext_vector_type(2)));

struct ForkArgs {
    uint32_t n, n_copies, n_codes, cov_on;
    const uint32_t *src, *dst_fall, *dst_jump;   // [n]
    const uint32_t *copy_fork, *copy_dst;        // [n_copies] fork index | FORK_COPY_JUMP, destination lane
    uint32_t *made, *cond, *jidx;                // [n]
};
#define FORK_COPY_JUMP 0x80000000u
#define FORK_GAS 10u   // JUMPI's gas, added by hand as the stepper does (no out-of-gas check)

// Forkability and jump resolution of lane s, the one predicate of mg_lanes_fork's
// contract: k_fork_check and the explorer's plan (lane_explore.cuh) both call it, so
// the two cannot drift.  False: s is not a forkable source.  True: cond = the
// condition's tag; jidx = the jump's instruction index when the jump is wanted and
// its target resolves to a JUMPDEST, else MG_JRES_NONE.
DEV bool fork_probe(const DevLanes &L, const DevSym &S, const DevCode *__restrict__ codes,
                    const uint8_t *__restrict__ a8, const uint32_t *__restrict__ a32, uint32_t n_codes, uint32_t s,
                    bool want_jump, uint32_t &cond, uint32_t &jidx) {
    const size_t N = L.N;
    cond = 0u; jidx = MG_JRES_NONE;
    const uint32_t flags = L.flags[s], sp = L.sp[s], cid = L.code_id[s], pc = L.pc[s];
    if (!(L.status[s] == MG_FORK && (flags & MG_LANE_SYMBOLIC) && !(flags & MG_LANE_TAINT) && sp >= 2u &&
          sp <= L.stack_cap && cid < n_codes && pc < codes[cid].n_instr))
        return false;
    const DevCode C = codes[cid];
    const uint32_t t_target = S.stag[(size_t)(sp - 1u) * N + s], t_cond = S.stag[(size_t)(sp - 2u) * N + s];
    if (!(t_target == 0u && t_cond != 0u)) return false;
    cond = t_cond;
    if (want_jump) {
        const U256 a = ld_word(gv(L.stack), (size_t)(sp - 1u) * N + s);
        if (u_fits32(a) && a.w[0] < C.n_jres) {
            const uint32_t idx = a32[C.jres_off + a.w[0]];
            if (idx < C.n_instr && a8[C.op_off + idx] == 0x5bu) jidx = idx;
        }
    }
    return true;
}

__global__ __launch_bounds__(256) void k_fork_check(DevLanes L, DevSym S, const DevCode *__restrict__ codes,
                                                    const uint8_t *__restrict__ a8,
                                                    const uint32_t *__restrict__ a32, ForkArgs F) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F.n) return;
    uint32_t made = MG_FORK_BAD_SRC, cond, jidx;
    if (fork_probe(L, S, codes, a8, a32, F.n_codes, F.src[i], F.dst_jump[i] != MG_FORK_NONE, cond, jidx))
        made = (F.dst_fall[i] != MG_FORK_NONE ? MG_FORK_MADE_FALL : 0u) | (jidx != MG_JRES_NONE ? MG_FORK_MADE_JUMP : 0u);
    F.made[i] = made; F.cond[i] = cond; F.jidx[i] = jidx;
}

// rows [w, rows) step G of a [row][lane][W] plane, lane s -> lane d; four rows in
// flight per thread (the loads of a batch are issued before its stores)
template <uint32_t W, class T>
DEV void fork_rows(T *plane, size_t N, uint32_t rows, uint32_t s, uint32_t d, uint32_t w, uint32_t G) {
    __attribute__((address_space(1))) T *p = (__attribute__((address_space(1))) T *)plane;
    uint32_t r = w;
    for (; (uint64_t)r + 3ull * G < rows; r += 4u * G) {
        T v[4][W];
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
#pragma unroll
            for (uint32_t k = 0; k < W; ++k) v[j][k] = p[((size_t)(r + j * G) * N + s) * W + k];
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
#pragma unroll
            for (uint32_t k = 0; k < W; ++k) p[((size_t)(r + j * G) * N + d) * W + k] = v[j][k];
    }
    for (; r < rows; r += G) {
        T v[W];
#pragma unroll
        for (uint32_t k = 0; k < W; ++k) v[k] = p[((size_t)r * N + s) * W + k];
#pragma unroll
        for (uint32_t k = 0; k < W; ++k) p[((size_t)r * N + d) * W + k] = v[k];
    }
}

// block (64, 4): x = the copy (sorted by destination lane), y = the row worker
__global__ __launch_bounds__(256) void k_fork_copy(DevLanes L, DevSym S, ForkArgs F) {
    const uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= F.n_copies) return;
    const uint32_t cf = F.copy_fork[c], f = cf & ~FORK_COPY_JUMP;
    const uint32_t m = F.made[f];
    if ((m & MG_FORK_BAD_SRC) || !(m & ((cf & FORK_COPY_JUMP) ? MG_FORK_MADE_JUMP : MG_FORK_MADE_FALL))) return;
    const uint32_t s = F.src[f], d = F.copy_dst[c];
    const uint32_t w = blockIdx.y * 4u + threadIdx.y, G = gridDim.y * 4u;
    const size_t N = L.N;
    // the source's live bounds (k_fork_check saw 2 <= sp <= stack_cap); every count
    // is clipped to its plane, so no state of a source can take a copy out of bounds
    const uint32_t n_stack = L.sp[s] - 2u;
    const uint32_t msize = min(L.msize[s], L.mem_cap);
    const uint32_t n_store = min(L.storage_count[s], L.storage_cap);
    fork_rows<2u>((v4u *)L.stack, N, n_stack, s, d, w, G);
    fork_rows<1u>(S.stag, N, n_stack, s, d, w, G);
    fork_rows<1u>(L.mem, N, (msize + 3u) / 4u, s, d, w, G);
    fork_rows<1u>(S.mtag, N, msize, s, d, w, G);
    fork_rows<4u>((v4u *)L.storage, N, n_store, s, d, w, G);
    fork_rows<1u>((v2u *)S.sttag, N, n_store, s, d, w, G);
    fork_rows<1u>((v4u *)S.node, N, min(S.n_nodes[s], S.node_cap), s, d, w, G);
    fork_rows<2u>((v4u *)S.cval, N, min(S.n_consts[s], S.const_cap), s, d, w, G);
    if (L.rec_cap) fork_rows<1u>(L.rec, N, min(L.rec_len[s], L.rec_cap), s, d, w, G);
    if (L.trace_cap) fork_rows<1u>(L.trace, N, min(L.trace_len[s], L.trace_cap), s, d, w, G);
    fork_rows<1u>(L.calldata, N, L.calldata_cap / 4u, s, d, w, G);
    fork_rows<2u>((v4u *)L.env, N, (uint32_t)MG_ENV_WORDS, s, d, w, G);
}

__global__ __launch_bounds__(256) void k_fork_commit(DevLanes L, DevSym S, const DevCode *__restrict__ codes,
                                                     const uint8_t *__restrict__ a8, uint8_t *__restrict__ cov,
                                                     ForkArgs F) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F.n) return;
    const uint32_t m = F.made[i];
    if ((m & MG_FORK_BAD_SRC) || m == 0u) return;
    const uint32_t s = F.src[i];
    // every scalar of the source, before any write (an in-place fall-through rewrites them)
    const uint32_t code_id = L.code_id[s], pc = L.pc[s], sp = L.sp[s], msize = L.msize[s], depth = L.depth[s];
    const uint32_t steps = L.steps[s], flags = L.flags[s], calldata_len = L.calldata_len[s];
    const uint32_t storage_count = L.storage_count[s], ret_offset = L.ret_offset[s], ret_len = L.ret_len[s];
    const uint32_t sha3_count = L.sha3_count[s], exp_count = L.exp_count[s], fent = L.fent[s];
    const uint32_t trace_len = L.trace_len[s], rec_len = L.rec_len[s];
    const uint32_t n_nodes = S.n_nodes[s], n_consts = S.n_consts[s];
    const uint64_t gas_min = L.gas_min[s], gas_max = L.gas_max[s], gas_limit = L.gas_limit[s];
    const DevCode C = codes[code_id];               // k_fork_check saw code_id and pc in range
    const uint8_t *__restrict__ gfent = a8 + C.fent_off;
    auto put = [&](uint32_t d, uint32_t npc, uint32_t nfent) {
        if (d != s) {
            L.code_id[d] = code_id; L.msize[d] = msize; L.calldata_len[d] = calldata_len;
            L.storage_count[d] = storage_count; L.ret_offset[d] = ret_offset; L.ret_len[d] = ret_len;
            L.sha3_count[d] = sha3_count; L.exp_count[d] = exp_count;
            L.trace_len[d] = trace_len; L.rec_len[d] = rec_len;
            S.n_nodes[d] = n_nodes; S.n_consts[d] = n_consts;
            L.gas_limit[d] = gas_limit;
        }
        L.pc[d] = npc; L.sp[d] = sp - 2u; L.depth[d] = depth + 1u;
        L.gas_min[d] = gas_min + FORK_GAS; L.gas_max[d] = gas_max + FORK_GAS;
        L.fent[d] = nfent; L.status[d] = MG_RUNNING; L.aux[d] = 0u; L.steps[d] = steps + 1u;
        L.flags[d] = flags & ~(uint32_t)MG_LANE_HOOK_ACK;
    };
    if (m & MG_FORK_MADE_JUMP) {
        const uint32_t idx = F.jidx[i];
        put(F.dst_jump[i], idx, (gfent[idx] & 1u) ? idx : fent);
    }
    if (m & MG_FORK_MADE_FALL) put(F.dst_fall[i], pc + 1u, (gfent[pc] & 2u) ? pc + 1u : fent);
    if (F.cov_on) cov[C.cov_off + pc] = 1;          // the reference marks every executed instruction
}
