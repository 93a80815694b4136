// bv_interp.cuh -- the body of kernel 2's interpreter kernels, included once per
// kernel (bv_eval.cuh) with BV_TERMS set: 0 = k_bv_eval (bit 0 of each program's
// result balloted into first_sat / sat_count / sat_bits), 1 = k_bv_terms (each
// lane's final accumulator stored to term_values[d][m]).  Textual inclusion, not
// a shared inlined function: k_bv_eval sits at its 64-VGPR budget, and as a
// template instance it was allocated differently (one VGPR spilled to scratch).
// No include guard: it is meant to be included more than once.
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    // instructions are read with scalar loads (uniform address -> s_load_dwordx4
    // through the scalar cache); LDS holds only the register slots.  Staging the
    // program tile in LDS measured slower (occupancy, ab/k2_lds_fetch.diff)
    uint4 *slots = smem;                         // [n_slots][2][BV_BLOCK]
    // group-major order with the tile count padded to a multiple of 8: the blocks
    // of one program tile share blockIdx % 8, i.e. one XCD's L2 (speed only)
    const uint32_t b = blockIdx.x;
    const uint32_t tile = tile_first + (b % tiles_pad);
    const uint32_t group = b / tiles_pad;
    if (tile >= tile_first + n_tiles) return;
    const uint32_t d0 = max(tile_dag[tile], dag_lo), d1 = min(tile_dag[tile + 1], dag_hi);
    if (d0 >= d1) return;
    // the tile is read from HBM once per block and reused for every model chunk
    const uint32_t i0 = prog_off[d0], i1 = prog_off[d1];
    // per-block results of the tile's DAGs: waves combine in LDS, the block adds
    // its totals to HBM once per DAG (not one atomic pair per wave per DAG)
#if !BV_TERMS
    __shared__ uint32_t blk_cnt[BV_TILE_DAGS], blk_first[BV_TILE_DAGS];
#endif
#if !BV_TERMS
    if (threadIdx.x < BV_TILE_DAGS) { blk_cnt[threadIdx.x] = 0u; blk_first[threadIdx.x] = 0xffffffffu; }
    __syncthreads();
#endif

    const uint32_t n_chunks = (n_models + BV_BLOCK - 1u) / BV_BLOCK;
    const uint32_t c_lo = group * chunks_per_block, c_hi = min(c_lo + chunks_per_block, n_chunks);
    // thread index = the wave's first (an SGPR) + the lane id (v_mbcnt): nothing
    // keeps threadIdx.x alive across the loops
    const uint32_t wave0 = uni(threadIdx.x) & ~63u;
    // this thread's column of the slot table (tid = m % BV_BLOCK = wave0 + lane for every
    // chunk): a slot access adds only the slot's uniform offset
    uint4 *const lane_slots = slots + wave0 + __lane_id();
    // DAG-major: one DAG's program (tens of instructions) is evaluated for all of
    // the block's model chunks while it is hot in the scalar cache; chunk-major
    // re-read the whole tile (up to 32 KiB) once per chunk, which the scalar
    // cache cannot hold and a CU's resident blocks' tiles overflow L2 with
    for (uint32_t d = d0; d < d1; ++d) {
    const uint32_t p0 = prog_off[d] - i0, p1 = prog_off[d + 1] - i0;
    for (uint32_t chunk = c_lo; chunk < c_hi; ++chunk) {
        BvCtx c{values, consts, lane_slots, n_models, chunk * BV_BLOCK + wave0 + __lane_id(), tab};
        U256 acc = u_zero();
        // byte offsets into the tile (32-bit, wave-uniform): the scalar load takes the
        // offset as its SGPR operand instead of a 64-bit address computed per instruction
        const char *const tileb = reinterpret_cast<const char *>(insns + i0);
        for (uint32_t off = p0 << 4, off_end = p1 << 4; off < off_end; off += 16u) {
            // c.m is the only per-lane context.  Round 3 hid its loop invariance
            // (an empty asm on it here) because min(m, n - 1) and m % 256 kept in
            // VGPRs across the loop spilled; with the predecoded dispatch the
            // kernel fits without it (62 VGPRs, no scratch) and runs 1.9 % faster
            // with them hoisted (profiles/r05/k2/ab_k2_q.log)
            uint32_t w0, ra, rb, rc;
            {
                const uint4 ins = *reinterpret_cast<const uint4 *>(tileb + uni(off));
                w0 = ins.x; ra = ins.y; rb = ins.z; rc = ins.w;
            }
            // op byte bit 7 = one operand (bv_predecode); w0 bit 30 = mask to width
            const uint32_t op = w0 & 0x3fu, width = (w0 >> 8) & 0x1ffu;
            if ((ra >> 30) != MG_BV_REF_ACC) acc = bv_fetch(c, ra);    // A in the accumulator's registers
            const U256 A = acc;
            U256 r;
            if (w0 & BV_W0_UNARY) {
                if (w0 & BV_W0_HOT) {
                    r = u_shr_u(A, rb & 0xffu, 0u);                              // MG_BV_EXTRACT
                } else {
                switch (op) {
                case MG_BV_NOT: r = u_not(A); break;
                case MG_BV_NEG: r = u_neg(A); break;
                case MG_BV_BNOT: r = u_small((A.w[0] & 1u) ^ 1u); break;
                case MG_BV_SEXT: r = bv_sext(A, rb); break;
                default: r = A; break;                                          // MG_BV_COPY, MG_BV_ZEXT
                }
                }
            } else {
                U256 B = bv_fetch(c, rb);
                if (w0 & BV_W0_HOT) {                        // BV_CMP_BAND
                    const uint32_t sub = (w0 >> 22) & 0x3fu;
                    bool t;
                    switch (sub) {
                    case MG_BV_EQ: t = bv_eq(A, B); break;
                    case MG_BV_NE: t = !bv_eq(A, B); break;
                    case MG_BV_ULT: t = u_lt(A, B); break;
                    case MG_BV_ULE: t = !u_lt(B, A); break;
                    case MG_BV_UGT: t = u_lt(B, A); break;
                    case MG_BV_UGE: t = !u_lt(A, B); break;
                    case MG_BV_SLT: t = u_slt(bv_sext(A, width), bv_sext(B, width)); break;
                    case MG_BV_SLE: t = !u_slt(bv_sext(B, width), bv_sext(A, width)); break;
                    case MG_BV_SGT: t = u_slt(bv_sext(B, width), bv_sext(A, width)); break;
                    default: t = !u_slt(bv_sext(A, width), bv_sext(B, width)); break;   // MG_BV_SGE
                    }
                    const U256 C = bv_fetch(c, rc);
                    r = u_small((t ? 1u : 0u) & C.w[0]);
                } else if (op == MG_BV_UDIV || op == MG_BV_UREM) {        // the unsigned division site
                    r = bv_udivrem(op == MG_BV_UDIV, A, B);
                } else if ((BV_DIV_OPS >> op) & 1ull) {      // the signed / overflow site
                    r = bv_divop(op, width, rc, A, B);
                } else {
                switch (op) {
                case MG_BV_ADD: r = u_add(A, B); break;
                case MG_BV_SUB: r = u_sub(A, B); break;
                case MG_BV_MUL: r = u_mul(A, B); break;
                case MG_BV_AND: r = u_and(A, B); break;
                case MG_BV_OR: r = u_or(A, B); break;
                case MG_BV_XOR: r = u_xor(A, B); break;
                case MG_BV_SHL: case MG_BV_LSHR: case MG_BV_ASHR: {
                    // a constant shift amount is wave-uniform: scalar-branch shifts
                    const bool ub = (rb >> 30) == MG_BV_REF_CONST;
                    const bool in = bv_fits32(B) && B.w[0] < width;
                    if (op == MG_BV_ASHR) {
                        const U256 sa = bv_sext(A, width);
                        const uint32_t fill = u_isneg(sa) ? 0xffffffffu : 0u;
                        if (ub) {
                            const uint32_t sh = uni(in ? B.w[0] : 255u);
                            r = u_shr_u(sa, sh, fill);
                        } else {
                            r = u_shr_n(sa, in ? B.w[0] : 255u, fill);
                        }
                    } else if (ub) {
                        if (!uni(in ? 1u : 0u)) r = u_zero();
                        else if (op == MG_BV_SHL) r = u_shl_u(A, uni(B.w[0]));
                        else r = u_shr_u(A, uni(B.w[0]), 0u);
                    } else {
                        r = !in ? u_zero() : op == MG_BV_SHL ? u_shl_n(A, B.w[0]) : u_shr_n(A, B.w[0], 0u);
                    }
                    break;
                }
                case MG_BV_EQ: r = u_small(bv_eq(A, B)); break;
                case MG_BV_NE: r = u_small(!bv_eq(A, B)); break;
                case MG_BV_ULT: r = u_small(u_lt(A, B)); break;
                case MG_BV_ULE: r = u_small(!u_lt(B, A)); break;
                case MG_BV_UGT: r = u_small(u_lt(B, A)); break;
                case MG_BV_UGE: r = u_small(!u_lt(A, B)); break;
                case MG_BV_SLT: r = u_small(u_slt(bv_sext(A, rc), bv_sext(B, rc))); break;
                case MG_BV_SLE: r = u_small(!u_slt(bv_sext(B, rc), bv_sext(A, rc))); break;
                case MG_BV_SGT: r = u_small(u_slt(bv_sext(B, rc), bv_sext(A, rc))); break;
                case MG_BV_SGE: r = u_small(!u_slt(bv_sext(A, rc), bv_sext(B, rc))); break;
                case MG_BV_BAND: r = u_small(A.w[0] & B.w[0] & 1u); break;
                case MG_BV_BOR: r = u_small((A.w[0] | B.w[0]) & 1u); break;
                case MG_BV_BXOR: r = u_small((A.w[0] ^ B.w[0]) & 1u); break;
                case MG_BV_BIMPLIES: r = u_small(((A.w[0] & 1u) ^ 1u) | (B.w[0] & 1u)); break;
                case MG_BV_ITE: {
                    const U256 C = bv_fetch(c, rc);
                    r = u_select((A.w[0] & 1u) != 0u, B, C);
                    break;
                }
                case MG_BV_CONCAT: r = u_or(u_shl_u(A, rc), B); break;                 // rc: uniform
                case MG_BV_ADD_NOOVF_U: {  // top bit of the (w+1)-bit sum is 0
                    const U256 s = u_add(A, B);
                    const bool ovf = rc >= 256u ? u_lt(s, A) : !bv_iszero(u_shr_u(s, rc, 0u));
                    r = u_small(!ovf);
                    break;
                }
                case MG_BV_SUB_NOUDF_U: r = u_small(!u_lt(A, B)); break;
                case MG_BV_TAB: r = bv_table(c, A, B, rc); break;
                case MG_BV_UMIN: r = u_select(u_lt(B, A), B, A); break;
                case MG_BV_UMAX: r = u_select(u_lt(A, B), B, A); break;
                case MG_BV_SMIN: r = u_select(u_slt(bv_sext(B, width), bv_sext(A, width)), B, A); break;
                case MG_BV_SMAX: r = u_select(u_slt(bv_sext(A, width), bv_sext(B, width)), B, A); break;
                case MG_BV_RSUB: r = u_sub(B, A); break;
                case MG_BV_RCONCAT: r = u_or(u_shl_u(B, rc), A); break;
                case BV_BIN2: {
                    const U256 t = bv_simple((w0 >> 22) & 0xfu, A, B);
                    const U256 C = bv_fetch(c, rc);
                    r = bv_simple((w0 >> 26) & 0xfu, t, C);
                    break;
                }
                case BV_BINX: {
                    uint32_t e0, e1, e2;
                    {
                        const uint4 x = *reinterpret_cast<const uint4 *>(tileb + uni(off + 16u));
                        e0 = x.x; e1 = x.y; e2 = x.z;
                    }
                    off += 16u;                              // the extension slot
                    const uint32_t k = (w0 >> 22) & 0x7u;
                    U256 t = bv_simple(e0 & 0xfu, A, B);
#pragma unroll 1
                    for (uint32_t j = 1; j < k; ++j) {
                        const uint32_t ref = j == 1u ? rc : j == 2u ? e1 : e2;
                        const U256 C = bv_fetch(c, ref);
                        t = bv_simple((e0 >> (4u * j)) & 0xfu, t, C);
                    }
                    r = t;
                    break;
                }
                case BV_EXT_RCAT: {
                    const uint32_t ew = (rc >> 17) & 0x1ffu;
                    U256 lo = u_shr_u(A, (rc >> 9) & 0xffu, 0u);
                    if (ew < 256u) lo = bv_mask(lo, ew);
                    r = u_or(u_shl_u(B, rc & 0x1ffu), lo);
                    break;
                }
                default: r = u_zero(); break;
                }
            }
            }
            // mask, fused tail and store in one test for the common instruction
            // that has none of them
            if (w0 & (BV_W0_MASK | (1u << 31) | (1u << 17))) {
                // the result masked to its width first (a tail's ops are 256-bit)
                if (w0 & BV_W0_MASK) r = bv_mask(r, width);
                if (w0 >> 31) {
                    // fused tail (bv_fuse): 1-3 bv_simple ops applied to this result,
                    // from an extension slot {kinds | count << 28, B1, B2, B3}
                    uint32_t e0, e1, e2, e3;
                    {
                        const uint4 x = *reinterpret_cast<const uint4 *>(tileb + uni(off + 16u));
                        e0 = x.x; e1 = x.y; e2 = x.z; e3 = x.w;
                    }
                    off += 16u;
                    const uint32_t k = e0 >> 28;
#pragma unroll 1
                    for (uint32_t j = 0; j < k; ++j) {
                        const uint32_t ref = j == 0u ? e1 : j == 1u ? e2 : e3;
                        const U256 C = bv_fetch(c, ref);
                        r = bv_simple((e0 >> (4u * j)) & 0xfu, r, C);
                    }
                }
                if ((w0 >> 17) & 1u) {
                    const uint32_t ds = (w0 >> 18) & 0xfu;
                    lane_slots[(ds * 2u) * BV_BLOCK] = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
                    lane_slots[(ds * 2u + 1u) * BV_BLOCK] = make_uint4(r.w[4], r.w[5], r.w[6], r.w[7]);
                }
            }
            acc = r;
        }
#if BV_TERMS
        // the term's value: lanes past the pool ran the program (uni() needs every
        // lane) and store nothing.  A 32-bit byte offset: bv_terms keeps the
        // buffer (DAGs x models x 32 bytes) under 4 GiB
        if (c.m < n_models) {
            uint4 *o = reinterpret_cast<uint4 *>(reinterpret_cast<char *>(term_values) + (d * n_models + c.m) * 32u);
            o[0] = make_uint4(acc.w[0], acc.w[1], acc.w[2], acc.w[3]);
            o[1] = make_uint4(acc.w[4], acc.w[5], acc.w[6], acc.w[7]);
        }
#else
        const bool sat = c.m < n_models && (acc.w[0] & 1u);
        const uint64_t bal = __ballot(sat);
        // the wave's first model, wave-uniform (an SGPR: nothing per lane stays live
        // across the DAG loop but c.m and the accumulator)
        const uint32_t wm = uni(c.m) & ~63u;
        if (bal && __lane_id() == 0u) {
            // optional per-model bitmap (one u64 per wave): lets the host replay
            // sequential check_quick_sat calls whose LRU bumps reorder the pool
            if (sat_bits) sat_bits[(size_t)d * bit_words + (wm >> 6)] = bal;
            atomicAdd(&blk_cnt[d - d0], (uint32_t)__popcll(bal));
            atomicMin(&blk_first[d - d0], wm + (uint32_t)(__ffsll((long long)bal) - 1));
        }
#endif
    }
    }
#if !BV_TERMS
    __syncthreads();
    const uint32_t tid = wave0 + __lane_id();
    if (tid < d1 - d0) {
        const uint32_t n = blk_cnt[tid], f = blk_first[tid];
        if (n) {
            atomicAdd(&sat_count[d0 + tid], n);
            atomicMin(&first_sat[d0 + tid], f);
        }
    }
#endif
