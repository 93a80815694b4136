// path_eval.cuh — mg_explore_check: a lane's recorded path evaluated straight from
// its expression arena against the candidate models (include/mythgpu.h states the
// contract; the fork filter of svm.py:319-326 with ModelCache.check_quick_sat,
// support_utils.py:60-68, as its question).
//
// Kernel 2's arrangement: one thread = one candidate model, one wave = one lane's
// arena for 64 models.  The node words, the constants, the path entries and the
// storage rows are read at wave-uniform addresses and every dispatch (kind,
// opcode, width, operand kind) is on scalars; only the 256-bit values are per
// thread.  A work item is (lane, group of 64-model chunks); a wave takes items in
// a grid-stride loop and reuses its slice of the workspace.
//
//   cone pass   wave-uniform, backwards from the path's condition nodes (a node
//               refers only to nodes below it): marks what the path needs in an LDS
//               bitmap and decides MG_PATH_UNKNOWN.  Every index followed later is
//               checked here, against the lane's own counts and the planes'
//               capacities; an unknown lane is never evaluated.  A KECCAK node's
//               input may be a tree of CONCAT nodes wider than 256 bits: the tree is
//               walked from the KECCAK node with a stack in LDS, its leaves (256 bits
//               at most) are marked, and the wide nodes themselves never are -- a
//               wide node marked any other way makes the lane unknown.
//   evaluation  marked nodes in ascending order; a node's value goes to the wave's
//               workspace slice [node][half][64 threads] as two uint4 per thread (a
//               dynamically indexed per-thread array would live in scratch) and is
//               read back by the same thread only.  A KECCAK node walks its tree
//               again, low part first, and assembles the table key (k0, k1) from the
//               leaves' values with shifts by wave-uniform amounts; wide nodes have no
//               workspace slot.
//   result      __ballot of "every entry holds", and-ed with the lineage's allowed
//               word; thread 0 writes the sat_bits word and the first model.
//
// The arithmetic is u256.cuh's and kernel 2's (bv_eval.cuh): bv_udivrem, bv_divop,
// bv_sext via u_slt, bv_mask, bv_table, and u256.cuh's z3 shifts.  Nothing here
// redefines x / 0, x mod 0, signed division or shifts >= the width.
#pragma once

#include "bv_eval.cuh"
#include "device_state.h"

#define PE_WAVE 64u
#define PE_TARGET_WAVES 2048u               // waves wanted per launch (8 per CU)
#define PE_MAX_WAVES 4096u
#define PE_WS_LIMIT (1ull << 30)            // workspace bytes one call may ask for
#define PE_MAX_LEAVES MG_PATH_KECCAK_LEAVES // leaves of a KECCAK input tree (= the walk's stack)

struct PathArgs {
    // the explore planes
    const uint32_t *path, *path_len, *root;
    uint32_t path_cap;
    // the call
    const mg_path_binding *bind;            // [n_bind]
    const uint32_t *lane_binding;           // [L.n]
    const unsigned long long *allowed;      // [n_bind][bit_words] or null
    const mg_path_functions *fn;            // the bound function tables (everything unbound: none)
    uint32_t n_bind, first, n, bit_words, chunks_per_item, groups;
    // the model pool (BvState)
    const uint4 *values;
    uint32_t n_models;
    BvTables tab;
    // workspace: [wave][ws_nodes][2][PE_WAVE] uint4
    uint4 *ws;
    uint32_t ws_nodes;
    // results
    uint32_t *first_sat;                    // [n], preset to MG_BV_NO_MODEL
    unsigned long long *sat_bits;           // [n][bit_words] or null
};

// the opcodes of MG_SYM_BIN / MG_SYM_UN the kernel evaluates (symbolic.binary / unary)
#define PE_BIN_OPS ((1u << 0x01) | (1u << 0x02) | (1u << 0x03) | (1u << 0x04) | (1u << 0x05) | (1u << 0x06) | \
                    (1u << 0x07) | (1u << 0x10) | (1u << 0x11) | (1u << 0x12) | (1u << 0x13) | (1u << 0x14) | \
                    (1u << 0x16) | (1u << 0x17) | (1u << 0x18) | (1u << 0x1a) | (1u << 0x1b) | (1u << 0x1c) | \
                    (1u << 0x1d))

// One lane of the image as the passes see it: every count already clipped to its
// plane's capacity, so an index below a count is an index inside the plane.
struct PeLane {
    uint32_t l, N, nn, nc, sc, symstore;
    const uint4 *node;                      // S.node  + l, row pitch N
    const uint4 *cval;                      // S.cval  + 2 l, row pitch 2 N
    const uint2 *sttag;                     // S.sttag + l, row pitch N
    const uint4 *storage;                   // L.storage + 4 l, row pitch 4 N
    uint32_t var_cdsize, tab_calldata, tab_storage;
    const uint32_t *var_env;                // the binding's five words
    const mg_path_functions *fn;
    uint2 *stk;                             // LDS [PE_MAX_LEAVES]: the tree walk's (ref, width)
};

DEV bool pe_marked(const uint32_t *marks, uint32_t k) { return (uni(marks[k >> 5]) >> (k & 31u)) & 1u; }
DEV void pe_mark(uint32_t *marks, uint32_t k) { marks[k >> 5] |= 1u << (k & 31u); }   // every thread, one value

// An operand ref of node k: a constant below the lane's count, or a node below k
// (marked).  False: the lane is unknown.
DEV bool pe_ref(const PeLane &A, uint32_t *marks, uint32_t k, uint32_t r) {
    if (r & MG_SYM_CONST) return (r & ~MG_SYM_CONST) < A.nc;
    if (r >= k) return false;
    pe_mark(marks, r);
    return true;
}

// The table bound for keccak256_<bits>, by scalar comparison with the bound widths.
DEV uint32_t pe_keccak_tab(const PeLane &A, uint32_t bits) {
    uint32_t tab = MG_PATH_UNBOUND;
    const uint32_t nk = min(uni(A.fn->n_keccak), MG_PATH_KECCAK_WIDTHS);
    for (uint32_t j = 0; j < nk; ++j)
        if (uni(A.fn->keccak_bits[j]) == bits) tab = uni(A.fn->keccak_tab[j]);
    return tab;
}

// The tree walk's stack: every thread writes the one value, the read is a scalar.
DEV void pe_push(uint2 *stk, uint32_t sp, uint32_t r, uint32_t width) { stk[sp] = make_uint2(r, width); }
DEV void pe_pop(const uint2 *stk, uint32_t sp, uint32_t &r, uint32_t &width) {
    const uint2 e = stk[sp];
    r = uni(e.x); width = uni(e.y);
}

// A reference of `width` bits inside a KECCAK input, made by node `parent`: a
// constant below the lane's count (256 bits at most) or a node below the parent.
DEV bool pe_tree_ref(const PeLane &A, uint32_t parent, uint32_t r, uint32_t width) {
    if (width == 0u || width > 512u) return false;
    if (r & MG_SYM_CONST) return width <= 256u && (r & ~MG_SYM_CONST) < A.nc;
    return r < parent;
}

// The cone pass of KECCAK node k's input (y, bits): every reference of the tree is
// below its referrer, every width is the one its referrer states, the tree has at
// most PE_MAX_LEAVES leaves; the leaves that are nodes are marked.  With
// leaves + sp <= PE_MAX_LEAVES throughout, the stack never outgrows its array.
DEV bool pe_cone_keccak(const PeLane &A, uint32_t *marks, uint32_t k, uint32_t y, uint32_t bits) {
    if (!pe_tree_ref(A, k, y, bits)) return false;
    uint32_t sp = 0u, leaves = 0u;
    pe_push(A.stk, sp++, y, bits);
    while (sp) {
        uint32_t r, ew;
        pe_pop(A.stk, --sp, r, ew);
        if (r & MG_SYM_CONST) { ++leaves; continue; }
        const uint4 nd = A.node[(size_t)r * A.N];
        const uint32_t kind = uni(nd.x) & 0xffu, width = uni(nd.x) >> 8, ny = uni(nd.y), nz = uni(nd.z), w = uni(nd.w);
        if (width != ew) return false;
        if (kind == MG_SYM_CONCAT && width > 256u) {
            const uint32_t wy = w & 0xffffu, wz = w >> 16;
            if (wy + wz != width || !pe_tree_ref(A, r, ny, wy) || !pe_tree_ref(A, r, nz, wz)) return false;
            if (leaves + sp + 2u > PE_MAX_LEAVES) return false;
            pe_push(A.stk, sp++, ny, wy);
            pe_push(A.stk, sp++, nz, wz);
            continue;
        }
        if (width > 256u) return false;
        pe_mark(marks, r);
        ++leaves;
    }
    return true;
}

// The cone pass's step for a marked node k: mark what it reads; false = unknown.
DEV bool pe_cone_node(const PeLane &A, uint32_t *marks, uint32_t k) {
    const uint4 nd = A.node[(size_t)k * A.N];
    const uint32_t kind = uni(nd.x) & 0xffu, width = uni(nd.x) >> 8, y = uni(nd.y), z = uni(nd.z), w = uni(nd.w);
    if (width == 0u || width > 256u) return false;
    const bool cd = A.var_cdsize != MG_PATH_UNBOUND && A.tab_calldata != MG_PATH_UNBOUND;
    switch (kind) {
    case MG_SYM_CDSIZE: return width == 256u && A.var_cdsize != MG_PATH_UNBOUND;
    case MG_SYM_ENV: return width == 256u && w < MG_ENV_WORDS && uni(A.var_env[w]) != MG_PATH_UNBOUND;
    case MG_SYM_CDLOAD: return width == 256u && cd && pe_ref(A, marks, k, y);
    case MG_SYM_CDBYTE: return width == 8u && cd;
    case MG_SYM_CDBYTEX: return width == 8u && cd && pe_ref(A, marks, k, y);
    case MG_SYM_BIN: {
        if (w == 0x0au) {                                   // EXP: Power(base y, exponent z)
            if (width != 256u || uni(A.fn->tab_power) == MG_PATH_UNBOUND) return false;
        } else if (w >= 32u || !((PE_BIN_OPS >> w) & 1u)) return false;
        if (!pe_ref(A, marks, k, y) || !pe_ref(A, marks, k, z)) return false;
        if (w == 0x1au) {                                   // BYTE: a constant index below 32
            if (!(y & MG_SYM_CONST)) return false;
            const uint4 *c = A.cval + (size_t)(y & ~MG_SYM_CONST) * 2u * A.N;
            const uint4 lo = c[0], hi = c[1];
            if (uni(lo.x) >= 32u || uni(lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) != 0u) return false;
        }
        return true;
    }
    case MG_SYM_UN: return (w == 0x15u || w == 0x19u) && pe_ref(A, marks, k, y);
    case MG_SYM_EXTRACT: {
        const uint32_t hi = w >> 16, lo = w & 0xffffu;
        if ((y & MG_SYM_CONST) || y >= k || lo > hi || width != hi - lo + 1u) return false;
        if (hi >= (uni(A.node[(size_t)y * A.N].x) >> 8)) return false;   // inside the source's width
        pe_mark(marks, y);
        return true;
    }
    case MG_SYM_CONCAT: {
        const uint32_t wy = w & 0xffffu, wz = w >> 16;
        return wy >= 1u && wz >= 1u && wy + wz == width && pe_ref(A, marks, k, y) && pe_ref(A, marks, k, z);
    }
    case MG_SYM_SLOAD: {
        if (width != 256u || z > A.sc || !pe_ref(A, marks, k, y)) return false;
        if (A.symstore && A.tab_storage == MG_PATH_UNBOUND) return false;
        for (uint32_t e = 0; e < z; ++e) {
            const uint2 tg = A.sttag[(size_t)e * A.N];
            const uint32_t kt = uni(tg.x), vt = uni(tg.y);
            if ((kt && kt - 1u >= k) || (vt && vt - 1u >= k)) return false;
            if (kt) pe_mark(marks, kt - 1u);
            if (vt) pe_mark(marks, vt - 1u);
        }
        return true;
    }
    case MG_SYM_KECCAK:
        return width == 256u && w >= 1u && w <= 512u && pe_keccak_tab(A, w) != MG_PATH_UNBOUND &&
               pe_cone_keccak(A, marks, k, y, w);
    default: return false;          // TERM, MLOADK, MSTOREK, BALANCE, anything else
    }
}

DEV U256 pe_ws_load(const uint4 *ws, uint32_t k) {
    const uint4 x = ws[(size_t)k * 2u * PE_WAVE], y = ws[((size_t)k * 2u + 1u) * PE_WAVE];
    U256 r;
    r.w[0] = x.x; r.w[1] = x.y; r.w[2] = x.z; r.w[3] = x.w;
    r.w[4] = y.x; r.w[5] = y.y; r.w[6] = y.z; r.w[7] = y.w;
    return r;
}
DEV void pe_ws_store(uint4 *ws, uint32_t k, const U256 &v) {
    ws[(size_t)k * 2u * PE_WAVE] = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    ws[((size_t)k * 2u + 1u) * PE_WAVE] = make_uint4(v.w[4], v.w[5], v.w[6], v.w[7]);
}
// an operand's value: the lane's constant (uniform address) or a node's value
DEV U256 pe_fetch(const PeLane &A, const uint4 *ws, uint32_t r) {
    if (r & MG_SYM_CONST) return ld2(A.cval + (size_t)(r & ~MG_SYM_CONST) * 2u * A.N);
    return pe_ws_load(ws, r);
}
DEV U256 pe_var(const BvCtx &c, uint32_t var) {
    return ld2(reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(c.values) +
                                               (var * c.n_models + c.model()) * 32u));
}

// The key (k0, k1) of KECCAK input (y, bits) under this thread's model: the leaves'
// values, low part first, each at its wave-uniform bit position; a part across bit
// 256 leaves its low bits in k0 and its high bits in k1.  The cone pass accepted the
// tree, so nothing is checked again.
DEV void pe_keccak_key(const PeLane &A, const uint4 *ws, uint32_t y, uint32_t bits, U256 &k0, U256 &k1) {
    k0 = u_zero(); k1 = u_zero();
    uint32_t sp = 0u, pos = 0u;
    pe_push(A.stk, sp++, y, bits);
    while (sp) {
        uint32_t r, ew;
        pe_pop(A.stk, --sp, r, ew);
        if (!(r & MG_SYM_CONST)) {
            const uint4 nd = A.node[(size_t)r * A.N];
            if ((uni(nd.x) & 0xffu) == MG_SYM_CONCAT && (uni(nd.x) >> 8) > 256u) {
                const uint32_t w = uni(nd.w);
                pe_push(A.stk, sp++, uni(nd.y), w & 0xffffu);           // high part: after the low one
                pe_push(A.stk, sp++, uni(nd.z), w >> 16);
                continue;
            }
        }
        const U256 v = bv_mask(pe_fetch(A, ws, r), ew);
        if (pos < 256u) {
            k0 = u_or(k0, u_shl_u(v, pos));
            if (pos + ew > 256u) k1 = u_or(k1, u_shr_u(v, 256u - pos, 0u));
        } else {
            k1 = u_or(k1, u_shl_u(v, pos - 256u));
        }
        pos += ew;
    }
}

// The value of node k under this thread's model (the cone pass accepted the node).
DEV U256 pe_eval_node(const PeLane &A, const BvCtx &c, const uint4 *ws, uint32_t k) {
    const uint4 nd = A.node[(size_t)k * A.N];
    const uint32_t kind = uni(nd.x) & 0xffu, width = uni(nd.x) >> 8, y = uni(nd.y), z = uni(nd.z), w = uni(nd.w);
    U256 r = u_zero();
    switch (kind) {
    case MG_SYM_CDSIZE: r = pe_var(c, A.var_cdsize); break;
    case MG_SYM_ENV: r = pe_var(c, uni(A.var_env[w])); break;
    case MG_SYM_CDLOAD: case MG_SYM_CDBYTE: case MG_SYM_CDBYTEX: {
        // calldata[i] = i < size (signed) ? the model's byte at i : 0; a CDLOAD is the
        // 32 bytes from value(y), one byte per trip of one loop
        const U256 size = pe_var(c, A.var_cdsize);
        U256 at = kind == MG_SYM_CDBYTE ? u_small(w) : pe_fetch(A, ws, y);
        if (kind == MG_SYM_CDBYTEX) at = u_add(at, u_small(w));
        const uint32_t nb = kind == MG_SYM_CDLOAD ? 32u : 1u;
#pragma unroll 1
        for (uint32_t j = 0; j < nb; ++j) {
            const U256 b = bv_mask(bv_table(c, at, u_zero(), A.tab_calldata), 8u);
            r = u_or(u_shl_u(r, 8u), u_select(u_slt(at, size), b, u_zero()));
            at = u_add(at, u_small(1));
        }
        break;
    }
    case MG_SYM_BIN: {
        const U256 a = pe_fetch(A, ws, y), b = pe_fetch(A, ws, z);
        switch (w) {
        case 0x01: r = u_add(a, b); break;
        case 0x02: r = u_mul(a, b); break;
        case 0x03: r = u_sub(a, b); break;
        case 0x04: case 0x06: r = bv_udivrem(w == 0x04u, a, b); break;                        // bvudiv, bvurem
        case 0x05: case 0x07: r = bv_divop(w == 0x05u ? MG_BV_SDIV : MG_BV_SREM, 256u, 0u, a, b); break;
        case 0x0a: r = bv_table(c, a, b, uni(A.fn->tab_power)); break;                         // Power(base y, exponent z)
        case 0x10: r = u_small(u_lt(a, b)); break;
        case 0x11: r = u_small(u_lt(b, a)); break;
        case 0x12: r = u_small(u_slt(a, b)); break;
        case 0x13: r = u_small(u_slt(b, a)); break;
        case 0x14: r = u_small(bv_eq(a, b)); break;
        case 0x16: r = u_and(a, b); break;
        case 0x17: r = u_or(a, b); break;
        case 0x18: r = u_xor(a, b); break;
        case 0x1a: r = bv_mask(u_shr_u(b, (31u - uni(a.w[0])) * 8u, 0u), 8u); break;        // a: constant < 32
        case 0x1b: r = u_shl(b, a); break;
        case 0x1c: r = u_lshr(b, a); break;
        default: r = u_ashr(b, a); break;                                                     // 0x1d
        }
        break;
    }
    case MG_SYM_UN: {
        const U256 a = pe_fetch(A, ws, y);
        r = w == 0x15u ? u_small(bv_iszero(a)) : u_not(a);
        break;
    }
    case MG_SYM_EXTRACT: r = u_shr_u(pe_ws_load(ws, y), w & 0xffffu, 0u); break;
    case MG_SYM_CONCAT: {
        const uint32_t wy = w & 0xffffu, wz = w >> 16;
        r = u_or(u_shl_u(bv_mask(pe_fetch(A, ws, y), wy), wz), bv_mask(pe_fetch(A, ws, z), wz));
        break;
    }
    case MG_SYM_KECCAK: {
        U256 k0, k1;
        pe_keccak_key(A, ws, y, w, k0, k1);
        r = bv_table(c, k0, k1, pe_keccak_tab(A, w));
        break;
    }
    default: {                                                                                // MG_SYM_SLOAD
        const U256 key = pe_fetch(A, ws, y);
        bool found = false;
        for (uint32_t e = z; e-- > 0u;) {               // newest first; SSTORE only appends
            const uint2 tg = A.sttag[(size_t)e * A.N];
            const uint32_t kt = uni(tg.x), vt = uni(tg.y);
            const uint4 *row = A.storage + (size_t)e * 4u * A.N;
            const U256 kv = kt ? pe_ws_load(ws, kt - 1u) : ld2(row);
            const bool hit = !found && bv_eq(kv, key);
            if (__ballot(hit)) {
                const U256 vv = vt ? pe_ws_load(ws, vt - 1u) : ld2(row + 2);
                r = u_select(hit, vv, r);
                found = found || hit;
            }
            if (!__ballot(!found)) break;
        }
        if (A.symstore && __ballot(!found)) r = u_select(found, r, bv_table(c, key, u_zero(), A.tab_storage));
        break;
    }
    }
    return bv_mask(r, width);
}

__global__ __launch_bounds__(PE_WAVE) void k_path_check(DevLanes L, DevSym S, PathArgs P) {
    extern __shared__ uint32_t pe_marks[];                  // one bit per node of the lane
    __shared__ uint2 pe_stack[PE_MAX_LEAVES];               // the walk of a KECCAK input tree
    const uint32_t t = __lane_id();
    const uint32_t N = L.N;
    uint4 *const ws = P.ws + (size_t)blockIdx.x * P.ws_nodes * 2u * PE_WAVE + t;
    const uint64_t total = (uint64_t)P.n * P.groups;
    for (uint64_t item = blockIdx.x; item < total; item += gridDim.x) {
        const uint32_t i = (uint32_t)(item / P.groups), g = (uint32_t)(item % P.groups);
        const uint32_t l = P.first + i;                     // < L.n: checked on the host
        const uint32_t c_lo = g * P.chunks_per_item, c_hi = min(c_lo + P.chunks_per_item, P.bit_words);
        // ---- the lane, every count clipped to its plane
        PeLane A;
        A.l = l; A.N = N;
        const uint32_t nn = uni(S.n_nodes[l]), plen = uni(P.path_len[l]), root = uni(P.root[l]);
        A.nn = nn;
        A.nc = min(uni(S.n_consts[l]), S.const_cap);
        A.sc = min(uni(L.storage_count[l]), L.storage_cap);
        A.symstore = uni(L.flags[l]) & MG_LANE_SYMSTORE;
        A.node = S.node + l; A.cval = S.cval + 2u * (size_t)l; A.sttag = S.sttag + l;
        A.storage = L.storage + 4u * (size_t)l;
        bool known = nn <= S.node_cap && nn <= P.ws_nodes && nn <= MG_PATH_MAX_NODES && plen <= P.path_cap &&
                     root < L.n;
        uint32_t b = MG_PATH_UNBOUND;
        if (known) b = uni(P.lane_binding[root]);
        known = known && b < P.n_bind;
        A.var_cdsize = A.tab_calldata = A.tab_storage = MG_PATH_UNBOUND;
        A.var_env = nullptr;
        A.fn = P.fn; A.stk = pe_stack;
        if (known) {
            const mg_path_binding *B = P.bind + b;
            A.var_cdsize = uni(B->var_cdsize); A.tab_calldata = uni(B->tab_calldata);
            A.tab_storage = uni(B->tab_storage); A.var_env = B->var_env;
        }
        // ---- cone pass
        if (known) {
            for (uint32_t w = 0; w < (nn + 31u) / 32u; ++w) pe_marks[w] = 0u;
            for (uint32_t e = 0; e < plen && known; ++e) {
                const uint32_t tag = uni(P.path[(size_t)e * N + l]) >> 1;
                if (tag == 0u || tag - 1u >= nn) known = false;
                else pe_mark(pe_marks, tag - 1u);
            }
            for (uint32_t k = nn; known && k-- > 0u;)
                if (pe_marked(pe_marks, k)) known = pe_cone_node(A, pe_marks, k);
        }
        if (!known) {
            if (t == 0u) {
                if (g == 0u) atomicMin(&P.first_sat[i], MG_PATH_UNKNOWN);
                if (P.sat_bits)
                    for (uint32_t c = c_lo; c < c_hi; ++c) P.sat_bits[(size_t)i * P.bit_words + c] = 0ull;
            }
            continue;
        }
        // ---- evaluation, one 64-model chunk at a time
        for (uint32_t chunk = c_lo; chunk < c_hi; ++chunk) {
            const BvCtx c{P.values, nullptr, nullptr, P.n_models, chunk * PE_WAVE + t, P.tab};
            for (uint32_t k = 0; k < nn; ++k)
                if (pe_marked(pe_marks, k)) pe_ws_store(ws, k, pe_eval_node(A, c, ws, k));
            bool sat = c.m < P.n_models;
            for (uint32_t e = 0; e < plen; ++e) {
                const uint32_t entry = uni(P.path[(size_t)e * N + l]);
                const bool nz = !bv_iszero(pe_ws_load(ws, (entry >> 1) - 1u));
                sat = sat && (nz == ((entry & 1u) != 0u));
            }
            unsigned long long ok = ~0ull;
            if (P.allowed) ok = P.allowed[(size_t)b * P.bit_words + chunk];
            const unsigned long long bal = __ballot(sat) & ok;
            if (t == 0u) {
                if (P.sat_bits) P.sat_bits[(size_t)i * P.bit_words + chunk] = bal;
                if (bal) atomicMin(&P.first_sat[i], chunk * PE_WAVE + (uint32_t)(__ffsll((long long)bal) - 1));
            }
        }
    }
}
