// run_table.h — kernel 1's straight-line run table, built by mg_load_code.
//
// Plain C++ (no HIP).  A straight-line run is PUSH/DUP/SWAP/POP/JUMPDEST, the
// pure ALU opcodes and the environment pushes (ADDRESS, ORIGIN, CALLER,
// CALLVALUE, GASPRICE, CALLDATASIZE, CODESIZE, GASLIMIT, PC, MSIZE: each pushes
// one lane constant at table gas, and memory cannot change inside a run),
// optionally closed by one JUMP or JUMPI.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace runtab {

enum : uint32_t {
    RUN_LEN_MAX = 64u,        // longest run (lane_step.cuh reads one pre-decoded word per wave lane)
    RX_CRE = 1u << 27,        // run table word x: the run escapes in a creation transaction
};

// Environment opcodes that push one lane constant at table gas.  RETURNDATASIZE
// is not one: it escapes on lanes that hold return data.
static inline bool env_push(uint32_t b) {
    return b == 0x30 || (b >= 0x32 && b <= 0x34) || b == 0x36 || b == 0x38 || b == 0x3a || b == 0x45 ||
           b == 0x58 || b == 0x59;
}

// Stack effect of a run-set opcode: words it needs, net change; false when the
// opcode is not in the run set.  env: the set includes the environment pushes.
static inline bool simple_op(uint32_t b, int &req, int &d, bool env) {
    if ((b >= 0x60 && b <= 0x7f) || (env && env_push(b))) { req = 0; d = 1; }
    else if (b >= 0x80 && b <= 0x8f) { req = (int)(b - 0x7f); d = 1; }
    else if (b >= 0x90 && b <= 0x9f) { req = (int)(b - 0x8e); d = 0; }
    else if (b == 0x50) { req = 1; d = -1; }
    else if (b == 0x5b) { req = 0; d = 0; }
    else if (b == 0x15 || b == 0x19) { req = 1; d = 0; }
    else if (b <= 0x03 && b >= 0x01) { req = 2; d = -1; }
    else if (b == 0x0b || (b >= 0x10 && b <= 0x1d)) { req = 2; d = -1; }
    else return false;
    return true;
}

// From every instruction, the run of simple opcodes that follows, at most
// RUN_LEN_MAX long, optionally ended by one JUMP or JUMPI, with the stack depth it
// needs, the growth it peaks at and the table gas of its simple part (jumps
// add their 8 / 10 by hand), so a lane can check once and execute the run
// without per-instruction checks.
// rx = len | need << 8 | peak << 16 | jump kind << 24 (1 JUMP, 2 JUMPI) | RX_CRE
// (the run holds CALLDATASIZE or CODESIZE, which a lane of a creation
// transaction does not execute), ry = table gas min | max << 16.
static inline void run_table(const uint8_t *ops, size_t ni, const uint32_t *gas_min, const uint32_t *gas_max,
                             bool env, std::vector<uint32_t> &rx, std::vector<uint32_t> &ry) {
    rx.assign(ni + 1, 0u);
    ry.assign(ni + 1, 0u);
    std::vector<int> need(ni + 1, 0), peak(ni + 1, 0), len(ni + 1, 0), jk(ni + 1, 0);
    std::vector<uint32_t> g0(ni + 1, 0u), g1(ni + 1, 0u);
    for (size_t i = ni; i-- > 0;) {
        const uint32_t b = ops[i];
        int req = -1, d = 0;
        if (b == 0x56 || b == 0x57) {               // a jump ends the run it closes
            len[i] = 1;
            need[i] = b == 0x56 ? 1 : 2;
            peak[i] = 0;
            jk[i] = b == 0x56 ? 1 : 2;
            g0[i] = g1[i] = 0u;
            rx[i] = 1u | ((uint32_t)need[i] << 8) | ((uint32_t)jk[i] << 24);
            ry[i] = 0u;
            continue;
        }
        if (!simple_op(b, req, d, env)) continue;   // not simple: runs end here
        const bool cont = len[i + 1] > 0 && len[i + 1] < (int)RUN_LEN_MAX;
        len[i] = 1 + (cont ? len[i + 1] : 0);
        need[i] = std::max(req, (cont ? need[i + 1] : 0) - d);
        peak[i] = std::max(0, d + (cont ? peak[i + 1] : 0));
        jk[i] = cont ? jk[i + 1] : 0;
        g0[i] = gas_min[b] + (cont ? g0[i + 1] : 0u);
        g1[i] = gas_max[b] + (cont ? g1[i + 1] : 0u);
        rx[i] = (uint32_t)len[i] | ((uint32_t)need[i] << 8) | ((uint32_t)peak[i] << 16) |
                ((uint32_t)jk[i] << 24) | ((b == 0x36 || b == 0x38) ? (uint32_t)RX_CRE : 0u) |
                (cont ? rx[i + 1] & RX_CRE : 0u);
        ry[i] = g0[i] | (g1[i] << 16);
    }
}

}  // namespace runtab
