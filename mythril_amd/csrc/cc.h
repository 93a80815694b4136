// Native conjunct compiler: kernel 2's register programs from lowered
// expression DAGs (host code, part of libmythgpu.so; C-ABI mg_cc_* in
// include/mythgpu.h).
//
// The host registers the nodes of lowered constraint DAGs once each (ids only
// grow: a DAG shared by many conjuncts -- a calldata word, a store chain -- is
// sent once), then asks for the program of one conjunct at a time.  The passes
// are mythril_amd/smt/flatten.py's, run over the native node table:
//   fold   ite(cmp(x, y), x, y) -> min/max; ite(x == y, x, y) -> y (interned)
//   emit   post-order, larger operand subtrees first, the conjunction of the
//          root folded conjunct by conjunct into one running result
//   slots  a result stays in the accumulator when its only reader is the next
//          instruction at an operand the accumulator may take (operand A, or B
//          of a commutative / swappable op), else a slot (linear scan, <= 16)
//   encode 4 x u32 per instruction (bv_eval.cuh)
// Ties between equal-size subtrees go to the lower node id (the Python pass
// breaks them by set order); every program computes the same truth value.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mythgpu.h"   // MG_BV_* opcodes, operand kinds and limits; MG_CC_*

namespace mgcc {

constexpr uint32_t WMAX = 256;
constexpr uint32_t NONE = 0xffffffffu;

inline bool is_cmp(uint32_t op) {
    return op == MG_BV_EQ || op == MG_BV_NE || (op >= MG_BV_ULT && op <= MG_BV_SGE) || op == MG_BV_ADD_NOOVF_U ||
           op == MG_BV_MUL_NOOVF_U || op == MG_BV_SUB_NOUDF_U;
}
inline bool commutative(uint32_t op) {
    switch (op) {
    case MG_BV_ADD: case MG_BV_MUL: case MG_BV_AND: case MG_BV_OR: case MG_BV_XOR: case MG_BV_EQ: case MG_BV_NE:
    case MG_BV_BAND: case MG_BV_BOR: case MG_BV_BXOR: case MG_BV_ADD_NOOVF_U: case MG_BV_MUL_NOOVF_U:
    case MG_BV_UMIN: case MG_BV_UMAX: case MG_BV_SMIN: case MG_BV_SMAX:
        return true;
    default:
        return false;
    }
}
// operand-swapped form (NONE: none)
inline uint32_t swapped(uint32_t op) {
    switch (op) {
    case MG_BV_ULT: return MG_BV_UGT; case MG_BV_UGT: return MG_BV_ULT;
    case MG_BV_ULE: return MG_BV_UGE; case MG_BV_UGE: return MG_BV_ULE;
    case MG_BV_SLT: return MG_BV_SGT; case MG_BV_SGT: return MG_BV_SLT;
    case MG_BV_SLE: return MG_BV_SGE; case MG_BV_SGE: return MG_BV_SLE;
    case MG_BV_SUB: return MG_BV_RSUB; case MG_BV_RSUB: return MG_BV_SUB;
    case MG_BV_CONCAT: return MG_BV_RCONCAT; case MG_BV_RCONCAT: return MG_BV_CONCAT;
    default: return NONE;
    }
}
inline bool acc_ok(uint32_t op, uint32_t k) { return k == 0 || (k == 1 && (commutative(op) || swapped(op) != NONE)); }

struct Node {
    uint32_t op, width, a0, n, imm;     // args: Compiler::args[a0 .. a0 + n)
};

struct Key {
    uint32_t op, width, imm;
    std::vector<uint32_t> args;
    bool operator==(const Key &o) const { return op == o.op && width == o.width && imm == o.imm && args == o.args; }
};
struct KeyHash {
    size_t operator()(const Key &k) const {
        uint64_t h = 1469598103934665603ull;
        auto mix = [&](uint64_t x) { h ^= x; h *= 1099511628211ull; };
        mix(k.op); mix(k.width); mix(k.imm);
        for (uint32_t a : k.args) mix(a);
        return (size_t)h;
    }
};

struct Virt {
    uint32_t op, width, imm;
    uint32_t nargs;
    // an operand: a leaf node id (is_virt = false) or an earlier instruction
    uint32_t arg[3];
    bool is_virt[3];
};

struct Compiler {
    std::vector<Node> nodes;
    std::vector<uint32_t> args;
    std::unordered_map<Key, uint32_t, KeyHash> intern;
    std::vector<uint32_t> fold_of;      // node -> folded node (NONE: not yet)
    std::vector<uint64_t> size_of;      // node -> operand-tree size + 1 (0: not yet)
    std::string err;

    uint32_t arg(uint32_t id, uint32_t k) const { return args[nodes[id].a0 + k]; }
    bool leaf(uint32_t id) const { return nodes[id].op == MG_CC_VAR || nodes[id].op == MG_CC_CONST; }

    uint32_t make(uint32_t op, uint32_t width, uint32_t imm, const std::vector<uint32_t> &a) {
        Key k{op, width, imm, a};
        auto it = intern.find(k);
        if (it != intern.end()) return it->second;
        const uint32_t id = (uint32_t)nodes.size();
        nodes.push_back(Node{op, width, (uint32_t)args.size(), (uint32_t)a.size(), imm});
        args.insert(args.end(), a.begin(), a.end());
        intern.emplace(std::move(k), id);
        fold_of.push_back(NONE);
        size_of.push_back(0);
        return id;
    }

    // rows: {op, width, first_arg, nargs, imm} x n; an argument is a node id, or
    // 0x80000000 | k for the k-th row of this same call.  ids[i] receives row i's
    // node id (an existing id when an equal node exists already: folding can
    // create a node the host registers later)
    int add(const uint32_t *rows, uint32_t n, const uint32_t *a, uint32_t na, uint32_t *ids) {
        std::vector<uint32_t> av;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t *r = rows + 5 * i;
            if (r[2] + (uint64_t)r[3] > na) { err = "argument range out of bounds"; return -1; }
            av.assign(a + r[2], a + r[2] + r[3]);
            for (uint32_t &x : av) {
                if (x & 0x80000000u) {
                    const uint32_t k = x & 0x7fffffffu;
                    if (k >= i) { err = "argument refers to a later row"; return -1; }
                    x = ids[k];
                } else if (x >= nodes.size()) {
                    err = "argument refers to an unregistered node";
                    return -1;
                }
            }
            ids[i] = make(r[0], r[1], r[4], av);
        }
        return 0;
    }

    // flatten._fold_select
    uint32_t fold(uint32_t root) {
        std::vector<std::pair<uint32_t, bool>> st{{root, false}};
        while (!st.empty()) {
            auto [x, ready] = st.back();
            st.pop_back();
            if (fold_of[x] != NONE) continue;
            const Node nd = nodes[x];
            if (nd.n == 0) { fold_of[x] = x; continue; }
            if (!ready) {
                st.push_back({x, true});
                for (uint32_t k = 0; k < nd.n; ++k)
                    if (fold_of[arg(x, k)] == NONE) st.push_back({arg(x, k), false});
                continue;
            }
            std::vector<uint32_t> a(nd.n);
            bool same = true;
            for (uint32_t k = 0; k < nd.n; ++k) { a[k] = fold_of[arg(x, k)]; same &= a[k] == arg(x, k); }
            uint32_t out = same ? x : make(nd.op, nd.width, nd.imm, a);
            if (nd.op == MG_BV_ITE && nd.width > 1) {
                const uint32_t c = a[0], p = a[1], q = a[2];
                const uint32_t cop = nodes[c].op;
                const bool minmax = cop >= MG_BV_ULT && cop <= MG_BV_SGE;
                if ((minmax || cop == MG_BV_EQ) && nodes[c].n == 2) {
                    const uint32_t cx = arg(c, 0), cy = arg(c, 1);
                    const bool fwd = cx == p && cy == q, rev = cy == p && cx == q;
                    if (fwd || rev) {
                        if (cop == MG_BV_EQ) {
                            out = q;
                        } else {
                            // (lo, hi) op per compare: ult/ule -> (umin, umax), ugt/uge ->
                            // (umax, umin), slt/sle -> (smin, smax), sgt/sge -> (smax, smin)
                            uint32_t lo, hi;
                            switch (cop) {
                            case MG_BV_ULT: case MG_BV_ULE: lo = MG_BV_UMIN; hi = MG_BV_UMAX; break;
                            case MG_BV_UGT: case MG_BV_UGE: lo = MG_BV_UMAX; hi = MG_BV_UMIN; break;
                            case MG_BV_SLT: case MG_BV_SLE: lo = MG_BV_SMIN; hi = MG_BV_SMAX; break;
                            default: lo = MG_BV_SMAX; hi = MG_BV_SMIN; break;
                            }
                            out = make(fwd ? lo : hi, nd.width, 0, {cx, cy});
                        }
                    }
                }
            }
            fold_of[x] = out;
            if (fold_of[out] == NONE) fold_of[out] = out;     // a folded node folds to itself
        }
        return fold_of[root];
    }

    uint64_t size(uint32_t root) {
        std::vector<std::pair<uint32_t, bool>> st{{root, false}};
        while (!st.empty()) {
            auto [x, ready] = st.back();
            st.pop_back();
            if (size_of[x] || leaf(x)) continue;
            if (!ready) {
                st.push_back({x, true});
                for (uint32_t k = 0; k < nodes[x].n; ++k) st.push_back({arg(x, k), false});
                continue;
            }
            uint64_t s = 1;                     // tree size (shared operands counted per use)
            for (uint32_t k = 0; k < nodes[x].n; ++k) {
                const uint32_t c = arg(x, k);
                const uint64_t sc = leaf(c) ? 0 : size_of[c] - 1;
                s = s + sc < s ? ~0ull - 1 : s + sc;    // saturating
            }
            size_of[x] = s + 1;                 // stored + 1 (0 = not yet)
        }
        return leaf(root) ? 0 : size_of[root] - 1;
    }
    uint64_t sz(uint32_t id) { return leaf(id) ? 0 : size(id); }

    // flatten.Compiler._lower for one node; returns false (err set) when unsupported
    bool lower_virt(uint32_t x, std::vector<Virt> &vs, std::unordered_map<uint32_t, uint32_t> &vid) {
        const Node nd = nodes[x];
        auto opnd = [&](Virt &v, uint32_t k, uint32_t c) {
            auto it = vid.find(c);
            if (it != vid.end()) { v.arg[k] = it->second; v.is_virt[k] = true; }
            else { v.arg[k] = c; v.is_virt[k] = false; }
        };
        if ((nd.op == MG_BV_BAND || nd.op == MG_BV_BOR) && nd.n > 2) {
            Virt v{nd.op, 1, 0, 2, {0, 0, 0}, {false, false, false}};
            opnd(v, 0, arg(x, 0));
            for (uint32_t k = 1; k < nd.n; ++k) {
                opnd(v, 1, arg(x, k));
                vs.push_back(v);
                v.arg[0] = (uint32_t)vs.size() - 1;
                v.is_virt[0] = true;
            }
            vid[x] = (uint32_t)vs.size() - 1;
            return true;
        }
        Virt v{nd.op, nd.width, 0, nd.n, {0, 0, 0}, {false, false, false}};
        if (nd.n > 3) { err = "operation with more than three operands"; return false; }
        if ((nd.op == MG_BV_BAND || nd.op == MG_BV_BOR) && nd.n == 1) {
            v.op = MG_BV_COPY;
            v.width = 1;
        } else if (nd.op == MG_BV_ZEXT && vid.count(arg(x, 0))) {
            vid[x] = vid[arg(x, 0)];            // values are kept masked: the same instruction
            return true;
        } else if (nd.op == MG_BV_EXTRACT) {
            v.imm = nd.imm;                      // low bit
        } else if (nd.op == MG_BV_SEXT) {
            v.imm = nodes[arg(x, 0)].width;
        } else if (nd.op == MG_BV_CONCAT) {
            v.imm = nodes[arg(x, 1)].width;
        } else if (is_cmp(nd.op)) {
            v.width = 1;
            v.imm = nodes[arg(x, 0)].width;
        } else if (nd.op == MG_BV_TAB) {
            v.imm = nd.imm;
        } else if (nd.op >= MG_BV_NUM_OPS) {
            err = "operation not evaluated on the device";
            return false;
        }
        for (uint32_t k = 0; k < nd.n; ++k) opnd(v, k, arg(x, k));
        vs.push_back(v);
        vid[x] = (uint32_t)vs.size() - 1;
        return true;
    }

    bool emit(uint32_t n, std::vector<Virt> &vs, std::unordered_map<uint32_t, uint32_t> &vid) {
        std::vector<std::pair<uint32_t, bool>> st{{n, false}};
        std::vector<uint32_t> kids;
        while (!st.empty()) {
            auto [x, ready] = st.back();
            st.pop_back();
            if (vid.count(x) || leaf(x)) continue;
            const Node nd = nodes[x];
            bool wide = nd.width > WMAX;
            for (uint32_t k = 0; k < nd.n; ++k) wide |= nodes[arg(x, k)].width > WMAX;
            if (wide) { err = "bit-vector wider than 256 bits"; return false; }
            if (!ready) {
                st.push_back({x, true});
                kids.clear();
                for (uint32_t k = 0; k < nd.n; ++k) {
                    const uint32_t c = arg(x, k);
                    if (!vid.count(c) && !leaf(c) && std::find(kids.begin(), kids.end(), c) == kids.end())
                        kids.push_back(c);
                }
                // ascending size (ties: lower id first), pushed smallest-first => computed largest-first
                std::sort(kids.begin(), kids.end(), [&](uint32_t a, uint32_t b) {
                    const uint64_t sa = sz(a), sb = sz(b);
                    return sa != sb ? sa < sb : a < b;
                });
                for (uint32_t c : kids) st.push_back({c, false});
                continue;
            }
            if (!lower_virt(x, vs, vid)) return false;
        }
        return true;
    }

    // returns the number of instructions, or -1 (unsupported, err set)
    int compile(uint32_t root0, std::vector<uint32_t> &out, uint32_t &max_slot) {
        if (root0 >= nodes.size()) { err = "unknown root"; return -1; }
        const uint32_t root = fold(root0);
        std::vector<Virt> vs;
        std::unordered_map<uint32_t, uint32_t> vid;
        std::vector<uint32_t> conj;
        if (nodes[root].op == MG_BV_BAND) for (uint32_t k = 0; k < nodes[root].n; ++k) conj.push_back(arg(root, k));
        else conj.push_back(root);
        bool have = false;
        uint32_t run = 0;
        bool run_virt = false;
        for (uint32_t c : conj) {
            if (!emit(c, vs, vid)) return -1;
            uint32_t cur;
            bool cur_virt;
            auto it = vid.find(c);
            if (it != vid.end()) { cur = it->second; cur_virt = true; }
            else { cur = c; cur_virt = false; }
            if (!have) {
                if (!cur_virt) {
                    Virt v{MG_BV_COPY, nodes[c].width, 0, 1, {c, 0, 0}, {false, false, false}};
                    vs.push_back(v);
                    cur = (uint32_t)vs.size() - 1;
                    cur_virt = true;
                }
                run = cur; run_virt = cur_virt; have = true;
            } else {
                Virt v{MG_BV_BAND, 1, 0, 2, {run, cur, 0}, {run_virt, cur_virt, false}};
                vs.push_back(v);
                run = (uint32_t)vs.size() - 1;
                run_virt = true;
            }
        }
        const uint32_t n = (uint32_t)vs.size();
        if (n > MG_BV_TILE_INSNS) { err = "program longer than one LDS tile"; return -1; }
        // uses of each instruction's result
        std::vector<std::vector<std::pair<uint32_t, uint32_t>>> uses(n);
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t k = 0; k < vs[i].nargs; ++k)
                if (vs[i].is_virt[k]) uses[vs[i].arg[k]].push_back({i, k});
        std::vector<uint32_t> slot_of(n, NONE), last_use(n, 0);
        std::vector<bool> needs(n, false);
        for (uint32_t j = 0; j < n; ++j) {
            if (uses[j].empty()) continue;
            bool need = uses[j].size() > 1;
            for (auto [i, k] : uses[j]) {
                need |= i != j + 1 || !acc_ok(vs[i].op, k);
                last_use[j] = std::max(last_use[j], i);
            }
            needs[j] = need;
        }
        std::vector<uint32_t> free_slots;
        for (int s = (int)MG_BV_MAX_SLOTS - 1; s >= 0; --s) free_slots.push_back((uint32_t)s);
        std::vector<std::vector<uint32_t>> expiring(n + 2);
        for (uint32_t i = 0; i < n; ++i) {
            for (uint32_t s : expiring[i]) free_slots.push_back(s);
            expiring[i].clear();
            if (!needs[i]) continue;
            if (free_slots.empty()) { err = "constraint set needs more than 16 live values"; return -1; }
            const uint32_t s = free_slots.back();
            free_slots.pop_back();
            slot_of[i] = s;
            max_slot = std::max(max_slot, s + 1);
            expiring[last_use[i] + 1].push_back(s);
        }
        out.assign((size_t)n * 4, 0u);
        for (uint32_t i = 0; i < n; ++i) {
            const Virt &v = vs[i];
            uint32_t refs[3] = {0, 0, 0};
            bool is_acc[3] = {false, false, false};
            for (uint32_t k = 0; k < v.nargs; ++k) {
                if (v.is_virt[k]) {
                    const uint32_t j = v.arg[k];
                    const bool acc = j + 1 == i && (k == 0 || slot_of[j] == NONE);
                    refs[k] = acc ? (MG_BV_REF_ACC << 30) : ((MG_BV_REF_SLOT << 30) | slot_of[j]);
                    is_acc[k] = acc;
                } else {
                    const Node &lf = nodes[v.arg[k]];
                    refs[k] = ((lf.op == MG_CC_CONST ? MG_BV_REF_CONST : MG_BV_REF_VAR) << 30) | lf.imm;
                }
            }
            uint32_t op = v.op;
            if (v.nargs > 1 && is_acc[1]) {
                std::swap(refs[0], refs[1]);
                std::swap(is_acc[0], is_acc[1]);
                if (!commutative(op)) op = swapped(op);
            }
            for (uint32_t k = 1; k < v.nargs; ++k)
                if (is_acc[k]) { err = "accumulator past operand A"; return -1; }
            uint32_t w0 = op | (v.width << 8);
            if (slot_of[i] != NONE) w0 |= (1u << 17) | (slot_of[i] << 18);
            uint32_t *w = &out[(size_t)i * 4];
            w[0] = w0;
            for (uint32_t k = 0; k < v.nargs; ++k) w[1 + k] = refs[k];
            if (v.op == MG_BV_EXTRACT || v.op == MG_BV_SEXT) w[2] = v.imm;
            else if (v.op == MG_BV_CONCAT || v.op == MG_BV_RCONCAT || is_cmp(v.op) || v.op == MG_BV_TAB) w[3] = v.imm;
        }
        return (int)n;
    }
};

}  // namespace mgcc
