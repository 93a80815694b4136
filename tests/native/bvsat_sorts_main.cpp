// A stand-alone driver for libmythsmt's sort checks (mythril_amd/csrc/bvsat.cpp):
// ill-sorted node tables, one or more per rule of include/mythsmt.h, and a few
// well-sorted queries, through ms_solve and through one ms_session.  Built with
// -fsanitize=address,undefined by tests/test_exact_words_cpu.py and run on its
// own: an operand read past its bits is a sanitizer report and a non-zero
// exit.  Exit status 0: every call returned what its row expects.
#include "../../include/mythsmt.h"

#include <cstdint>
#include <cstdio>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

namespace {

struct Query {
    std::vector<uint32_t> nodes, args, limbs{0u}, roots;
    uint32_t base, n_vars;
    explicit Query(uint32_t node_base = 0, uint32_t var_base = 0) : base(node_base), n_vars(var_base) {}

    uint32_t node(uint32_t op, uint32_t w, std::initializer_list<uint32_t> as, uint32_t p0 = 0, uint32_t p1 = 0) {
        uint32_t row[6] = {op, w, (uint32_t)as.size(), (uint32_t)args.size(), p0, p1};
        args.insert(args.end(), as.begin(), as.end());
        nodes.insert(nodes.end(), row, row + 6);
        return base + (uint32_t)(nodes.size() / 6) - 1;
    }
    uint32_t var(uint32_t w) { return node(MS_VAR, w, {}, n_vars++); }
    uint32_t cst(uint32_t w, uint64_t v) {
        uint32_t at = (uint32_t)limbs.size();
        for (uint32_t i = 0; i < (w + 31) / 32; ++i) limbs.push_back(i < 2 ? (uint32_t)(v >> (32 * i)) : 0u);
        return node(MS_CONST, w, {}, at);
    }
    uint32_t array(uint32_t id, uint32_t range) { return node(MS_ARRAY, 0, {}, id, range); }
    // a word as a root: w-bit e != 0
    void nonzero(uint32_t e, uint32_t w) { roots.push_back(node(MS_DISTINCT, 1, {e, cst(w, 0)})); }
    void root(uint32_t e) { roots.push_back(e); }
    ms_query q() {
        if (args.empty()) args.push_back(0u);
        ms_query out = {(uint32_t)(nodes.size() / 6), nodes.data(), args.data(), limbs.data(), (uint32_t)roots.size(),
                        roots.data(), 0u, nullptr, n_vars, 4u, 4u};
        return out;
    }
};

struct Row {
    std::string label;
    int want;
    std::function<void(Query &)> build;
};

std::vector<Row> rows() {
    std::vector<Row> r;
    auto bad = [&](const char *label, std::function<void(Query &)> f) { r.push_back({label, MS_EINVAL, f}); };
    // operand count per opcode
    bad("bvadd of one operand", [](Query &q) { q.nonzero(q.node(MS_BVADD, 8, {q.var(8)}), 8); });
    bad("bvnot of two operands", [](Query &q) { q.nonzero(q.node(MS_BVNOT, 8, {q.var(8), q.var(8)}), 8); });
    bad("bvult of one operand", [](Query &q) { q.root(q.node(MS_BVULT, 1, {q.var(8)})); });
    bad("eq of three operands", [](Query &q) { q.root(q.node(MS_EQ, 1, {q.var(8), q.var(8), q.var(8)})); });
    bad("not of two operands", [](Query &q) { q.root(q.node(MS_NOT, 1, {q.var(1), q.var(1)})); });
    bad("ite of two operands", [](Query &q) { q.nonzero(q.node(MS_ITE, 8, {q.var(1), q.var(8)}), 8); });
    bad("concat of one operand", [](Query &q) { q.nonzero(q.node(MS_CONCAT, 8, {q.var(8)}), 8); });
    bad("extract of two operands", [](Query &q) { q.nonzero(q.node(MS_EXTRACT, 4, {q.var(8), q.var(8)}, 3, 0), 4); });
    bad("select of one operand", [](Query &q) { q.nonzero(q.node(MS_SELECT, 8, {q.array(0, 8)}), 8); });
    bad("a constant with an operand", [](Query &q) { q.nonzero(q.node(MS_CONST, 8, {q.var(8)}, 0), 8); });
    // arithmetic, bitwise and shift operators
    static const uint32_t word_ops[] = {MS_BVADD, MS_BVSUB, MS_BVMUL, MS_BVUDIV, MS_BVUREM, MS_BVSDIV, MS_BVSREM,
                                        MS_BVSMOD, MS_BVAND, MS_BVOR, MS_BVXOR, MS_BVSHL, MS_BVLSHR, MS_BVASHR};
    for (uint32_t op : word_ops) {
        bad("word operator, narrower second operand", [op](Query &q) { q.nonzero(q.node(op, 8, {q.var(8), q.var(4)}), 8); });
        bad("word operator, wider second operand", [op](Query &q) { q.nonzero(q.node(op, 8, {q.var(8), q.var(16)}), 8); });
        bad("word operator, narrower first operand", [op](Query &q) { q.nonzero(q.node(op, 8, {q.var(4), q.var(8)}), 8); });
        bad("word operator, node wider than both", [op](Query &q) { q.nonzero(q.node(op, 16, {q.var(8), q.var(8)}), 16); });
        bad("word operator, node narrower than both", [op](Query &q) { q.nonzero(q.node(op, 4, {q.var(8), q.var(8)}), 4); });
    }
    bad("bvneg of a narrower operand", [](Query &q) { q.nonzero(q.node(MS_BVNEG, 8, {q.var(4)}), 8); });
    bad("bvnot of a wider operand", [](Query &q) { q.nonzero(q.node(MS_BVNOT, 8, {q.var(16)}), 8); });
    bad("a word operator on an array", [](Query &q) { q.nonzero(q.node(MS_BVNOT, 8, {q.array(0, 8)}), 8); });
    // comparisons and the overflow predicates
    static const uint32_t cmp_ops[] = {MS_EQ, MS_DISTINCT, MS_BVULT, MS_BVULE, MS_BVUGT, MS_BVUGE, MS_BVSLT, MS_BVSLE,
                                       MS_BVSGT, MS_BVSGE, MS_BVADD_NOOVFL_U, MS_BVUMUL_NOOVFL, MS_BVSUB_NOUDFL_U};
    for (uint32_t op : cmp_ops) {
        bad("comparison, narrower second operand", [op](Query &q) { q.root(q.node(op, 1, {q.var(8), q.var(4)})); });
        bad("comparison, wider second operand", [op](Query &q) { q.root(q.node(op, 1, {q.var(8), q.var(16)})); });
        bad("comparison of width 2", [op](Query &q) { q.nonzero(q.node(op, 2, {q.var(8), q.var(8)}), 2); });
    }
    // Boolean connectives
    bad("and with an 8-bit operand", [](Query &q) { q.root(q.node(MS_AND, 1, {q.var(1), q.var(8)})); });
    bad("or without operands", [](Query &q) { q.root(q.node(MS_OR, 1, {})); });
    bad("not of an 8-bit operand", [](Query &q) { q.root(q.node(MS_NOT, 1, {q.var(8)})); });
    bad("xor with an array operand", [](Query &q) { q.root(q.node(MS_XOR, 1, {q.var(1), q.array(0, 8)})); });
    bad("implies with a 4-bit operand", [](Query &q) { q.root(q.node(MS_IMPLIES, 1, {q.var(4), q.var(1)})); });
    // ite
    bad("ite with an 8-bit condition", [](Query &q) { q.nonzero(q.node(MS_ITE, 8, {q.var(8), q.var(8), q.var(8)}), 8); });
    bad("ite with a narrower arm", [](Query &q) { q.nonzero(q.node(MS_ITE, 8, {q.var(1), q.var(8), q.var(4)}), 8); });
    bad("ite with a wider arm", [](Query &q) { q.nonzero(q.node(MS_ITE, 8, {q.var(1), q.var(16), q.var(8)}), 8); });
    // concat, extensions, extract
    bad("concat[16] of 8 and 4 bits", [](Query &q) { q.nonzero(q.node(MS_CONCAT, 16, {q.var(8), q.var(4)}), 16); });
    bad("concat[16] of 8 and 16 bits", [](Query &q) { q.nonzero(q.node(MS_CONCAT, 16, {q.var(8), q.var(16)}), 16); });
    bad("zero_extend[16] by 8 of 4 bits", [](Query &q) { q.nonzero(q.node(MS_ZERO_EXTEND, 16, {q.var(4)}, 8), 16); });
    bad("zero_extend[16] by 8 of 16 bits", [](Query &q) { q.nonzero(q.node(MS_ZERO_EXTEND, 16, {q.var(16)}, 8), 16); });
    bad("sign_extend[16] by 8 of 4 bits", [](Query &q) { q.nonzero(q.node(MS_SIGN_EXTEND, 16, {q.var(4)}, 8), 16); });
    bad("sign_extend[16] by 8 of 16 bits", [](Query &q) { q.nonzero(q.node(MS_SIGN_EXTEND, 16, {q.var(16)}, 8), 16); });
    bad("extract[4] of bits 7..0", [](Query &q) { q.nonzero(q.node(MS_EXTRACT, 4, {q.var(8)}, 7, 0), 4); });
    bad("extract[8] of bits 3..0", [](Query &q) { q.nonzero(q.node(MS_EXTRACT, 8, {q.var(8)}, 3, 0), 8); });
    bad("extract[8] of bits 11..4 of 8 bits", [](Query &q) { q.nonzero(q.node(MS_EXTRACT, 8, {q.var(8)}, 11, 4), 8); });
    bad("extract with lo > hi", [](Query &q) { q.nonzero(q.node(MS_EXTRACT, 2, {q.var(8)}, 2, 3), 2); });
    // arrays
    bad("select at a narrower index than the store below it", [](Query &q) {
        uint32_t s = q.node(MS_STORE, 0, {q.array(0, 8), q.var(8), q.var(8)}, 0, 8);
        q.nonzero(q.node(MS_SELECT, 8, {s, q.var(4)}), 8);
    });
    bad("select at a wider index than the store below it", [](Query &q) {
        uint32_t s = q.node(MS_STORE, 0, {q.array(0, 8), q.var(8), q.var(8)}, 0, 8);
        q.nonzero(q.node(MS_SELECT, 8, {s, q.var(16)}), 8);
    });
    bad("two reads of one array, the second index narrower", [](Query &q) {
        uint32_t a = q.array(0, 8);
        q.nonzero(q.node(MS_SELECT, 8, {a, q.var(8)}), 8);
        q.nonzero(q.node(MS_SELECT, 8, {a, q.var(4)}), 8);
    });
    bad("two reads of one array, the second index wider", [](Query &q) {
        uint32_t a = q.array(0, 8);
        q.nonzero(q.node(MS_SELECT, 8, {a, q.var(8)}), 8);
        q.nonzero(q.node(MS_SELECT, 8, {a, q.var(16)}), 8);
    });
    bad("select[4] of an array of bytes", [](Query &q) { q.nonzero(q.node(MS_SELECT, 4, {q.array(0, 8), q.var(8)}), 4); });
    bad("select[16] of an array of bytes", [](Query &q) { q.nonzero(q.node(MS_SELECT, 16, {q.array(0, 8), q.var(8)}), 16); });
    bad("a stored value wider than the range", [](Query &q) {
        uint32_t s = q.node(MS_STORE, 0, {q.array(0, 8), q.var(8), q.var(16)}, 0, 8);
        q.nonzero(q.node(MS_SELECT, 8, {s, q.var(8)}), 8);
    });
    bad("select of a word", [](Query &q) { q.nonzero(q.node(MS_SELECT, 8, {q.var(8), q.var(8)}), 8); });
    bad("a constant array of a narrower default", [](Query &q) {
        uint32_t k = q.node(MS_K, 0, {q.cst(4, 1)}, 0, 8);
        uint32_t s = q.node(MS_STORE, 0, {k, q.var(8), q.var(8)}, 0, 8);
        q.nonzero(q.node(MS_SELECT, 8, {s, q.var(8)}), 8);
    });
    // function applications
    bad("a second application at a narrower argument", [](Query &q) {
        q.nonzero(q.node(MS_UF, 8, {q.var(8)}, 1), 8);
        q.nonzero(q.node(MS_UF, 8, {q.var(4)}, 1), 8);
    });
    bad("a second application at a wider argument", [](Query &q) {
        q.nonzero(q.node(MS_UF, 8, {q.var(8)}, 1), 8);
        q.nonzero(q.node(MS_UF, 8, {q.var(16)}, 1), 8);
    });
    bad("a second application of a narrower range", [](Query &q) {
        q.nonzero(q.node(MS_UF, 8, {q.var(8)}, 1), 8);
        q.nonzero(q.node(MS_UF, 4, {q.var(8)}, 1), 4);
    });
    bad("a second application with one more argument", [](Query &q) {
        q.nonzero(q.node(MS_UF, 8, {q.var(8)}, 1), 8);
        q.nonzero(q.node(MS_UF, 8, {q.var(8), q.var(8)}, 1), 8);
    });
    // the mixed-width kernel-2 program that read out of bounds:
    // a64 == c1, b256 == c2, bvxor(bvmul(sign_extend[200](a64), b256), sign_extend[200](a64)) != v
    bad("bvxor[256](bvmul[256](sign_extend[200](a64), b256), sign_extend[200](a64))", [](Query &q) {
        uint32_t a = q.var(64), b = q.var(256);
        q.root(q.node(MS_EQ, 1, {a, q.cst(64, 0x8000000000000001ull)}));
        q.root(q.node(MS_EQ, 1, {b, q.cst(256, 0x123456789abcdef1ull)}));
        uint32_t sx = q.node(MS_SIGN_EXTEND, 200, {a}, 136);
        uint32_t e = q.node(MS_BVXOR, 256, {q.node(MS_BVMUL, 256, {sx, b}), sx});
        q.root(q.node(MS_DISTINCT, 1, {e, q.cst(256, 5)}));
    });
    // well-sorted queries
    r.push_back({"x + 1 == x at 33 bits", MS_UNSAT, [](Query &q) {
        uint32_t x = q.var(33);
        q.root(q.node(MS_EQ, 1, {q.node(MS_BVADD, 33, {x, q.cst(33, 1)}), x}));
    }});
    r.push_back({"x * 3 == 7 at 31 bits", MS_SAT, [](Query &q) {
        q.root(q.node(MS_EQ, 1, {q.node(MS_BVMUL, 31, {q.var(31), q.cst(31, 3)}), q.cst(31, 7)}));
    }});
    r.push_back({"select(store(m, i, v), i) != v", MS_UNSAT, [](Query &q) {
        uint32_t i = q.var(8), v = q.var(8);
        uint32_t s = q.node(MS_STORE, 0, {q.array(0, 8), i, v}, 0, 8);
        q.root(q.node(MS_DISTINCT, 1, {q.node(MS_SELECT, 8, {s, i}), v}));
    }});
    r.push_back({"sign_extend[200](a64) >>a 199 == all ones, a64 negative", MS_SAT, [](Query &q) {
        uint32_t a = q.var(64);
        uint32_t sx = q.node(MS_SIGN_EXTEND, 200, {a}, 136);
        uint32_t sh = q.node(MS_BVASHR, 200, {sx, q.cst(200, 199)});
        q.root(q.node(MS_EQ, 1, {sh, q.node(MS_BVNOT, 200, {q.cst(200, 0)})}));
    }});
    return r;
}

}  // namespace

int main() {
    const ms_limits lim = {50000u, 20000u, 1000u};
    std::vector<uint32_t> model(1 << 12);
    int failures = 0;
    const std::vector<Row> all = rows();
    // each row alone through ms_solve
    for (const Row &row : all) {
        Query q;
        row.build(q);
        ms_query mq = q.q();
        uint32_t len = 0;
        int rc = ms_solve(&mq, &lim, model.data(), (uint32_t)model.size(), &len, nullptr);
        if (rc != row.want) {
            std::printf("ms_solve: %s: returned %d, expected %d\n", row.label.c_str(), rc, row.want);
            ++failures;
        }
    }
    // all rows through one session: a rejected query leaves the session's node
    // table as it found it, so the next query's node ids continue from the
    // last accepted one and the well-sorted rows at the end are still decided
    ms_session *s = nullptr;
    if (ms_session_open(&s) != 0 || !s) {
        std::printf("ms_session_open failed\n");
        return 2;
    }
    uint32_t node_base = 0, var_base = 0;
    for (size_t pass = 0; pass < 2; ++pass)
        for (const Row &row : all) {
            Query q(node_base, var_base);
            row.build(q);
            ms_query mq = q.q();
            uint32_t len = 0;
            int rc = ms_session_solve(s, &mq, &lim, model.data(), (uint32_t)model.size(), &len, nullptr);
            if (rc != row.want) {
                std::printf("ms_session_solve (pass %zu): %s: returned %d, expected %d\n", pass, row.label.c_str(), rc,
                            row.want);
                ++failures;
            }
            if (rc != MS_EINVAL) {
                node_base += mq.n_nodes;
                var_base = q.n_vars;
            }
        }
    ms_session_close(s);
    std::printf("%zu rows, %d failures\n", all.size(), failures);
    return failures ? 1 : 0;
}
