// device_state.h — HBM layout of a lane batch and of loaded codes.
//
// Lane state is interleaved by lane so that the 64 lanes of a wave that sit at
// the same pc / stack depth touch one contiguous span per access:
//   stack    [slot][lane]      32-byte word per lane   (2 x dwordx4 per access)
//   memory   [dword][lane]     big-endian dword: EVM byte 4d+0 in bits 31..24
//   calldata [dword][lane]     same packing as memory
//   env      [word][lane]      32 bytes
//   storage  [slot][lane]      64 bytes: key limbs 0..7, value limbs 8..15
// Scalars are one array per field.  A 256-bit word is 8 little-endian u32 limbs.
#pragma once
#include <stdint.h>

#include "../../include/mythgpu.h"   // MG_FENT_NONE

struct DevLanes {
    uint32_t n;          // lanes in the batch
    uint32_t N;          // row pitch in lanes (n rounded up to 64)
    uint32_t stack_cap, mem_cap, calldata_cap, storage_cap;
    // scalars [N]
    uint32_t *code_id, *pc, *sp, *msize, *depth, *status, *aux, *steps, *flags;
    uint32_t *calldata_len, *storage_count, *ret_offset, *ret_len;
    uint32_t *sha3_count, *exp_count;
    uint64_t *gas_min, *gas_max, *gas_limit;
    // interleaved state
    uint4 *stack;        // [stack_cap][N][2]
    uint32_t *mem;       // [mem_cap/4][N]
    uint32_t *calldata;  // [calldata_cap/4][N]
    uint4 *env;          // [5][N][2]
    uint4 *storage;      // [storage_cap][N][4]
    // instruction traces (BoundedLoopsStrategy): address per popped instruction
    uint32_t trace_cap;
    uint32_t *trace_len; // [N]
    uint32_t *trace;     // [trace_cap][N]
    // function-manager records (MG_REC_*): uint32 words per lane, in execution order
    uint32_t rec_cap;
    uint32_t *rec_len;   // [N]
    uint32_t *rec;       // [rec_cap][N]
    // active_function_name (svm.py:575-637): index of the last JUMP / JUMPI landing
    // on a function entry since the upload, MG_FENT_NONE if none
    uint32_t *fent;      // [N]
};

// Symbolic planes (mg_sym_alloc): stack tags, expression arena, constants.
struct DevSym {
    uint32_t node_cap, const_cap;
    uint32_t *stag;      // [stack_cap][N]
    uint4 *node;         // [node_cap][N]
    uint4 *cval;         // [const_cap][N][2]
    uint32_t *n_nodes, *n_consts;   // [N]
    uint32_t *mtag;      // [mem_cap][N]  memory byte tags: 0, or 1 + (node << 5 | byte j)
    uint2 *sttag;        // [storage_cap][N]  storage chain entry (key, value) tags: 0 or 1 + node
};

// Taint planes (mg_taint_alloc): object handle per stack slot, annotation mask
// per object, the lane's atom count, sink and yield-class masks.
struct DevTaint {
    uint32_t obj_cap;
    const uint32_t *prog;              // [256] action word per opcode (mg_taint_program)
    const uint8_t *force;              // per code instruction (coverage layout): 1 = the host runs
                                       // this instruction's hooks (mg_taint_force), or null
    uint32_t *sobj;                    // [stack_cap][N]
    unsigned long long *omask;         // [obj_cap][N]
    uint32_t *oremap;                  // [obj_cap][N] scratch of the handle compaction
    uint32_t *n_obj, *n_fixed, *n_atoms, *tflags;   // [N] (handles below n_fixed are the host's)
    unsigned long long *sink, *ymask;          // [N]
};

// Resident initial image of a batch (mg_lanes_reset); passed to the stepping
// kernel when it re-initialises every lane itself before stepping
// (mg_run_batches), pc == nullptr otherwise.  The kernels only read it; the
// pointers are not const because the context keeps this struct and every
// upload writes the planes (the second destination of these fields).
struct DevResetImage {
    uint32_t *pc, *depth, *status, *aux, *steps, *storage_count;
    uint64_t *gas_min, *gas_max;
    uint4 *storage;
};

// One loaded code (Disassembly): arrays live in one device arena.
struct DevCode {
    uint32_t n_instr;    // len(instruction_list)
    uint32_t n_bytes;    // len(bytecode) for CODESIZE / CODECOPY
    uint32_t n_jres;     // entries of the jump-resolve table (last address + 1)
    uint32_t op_off;     // u8  [n_instr]            opcode byte (0xfe = INVALID)
    uint32_t addr_off;   // u32 [n_instr]            byte address of instruction
    uint32_t push_off;   // u32 [n_instr][8]         push immediate (limbs)
    uint32_t jres_off;   // u32 [n_jres]             first index with addr >= t
    uint32_t bytes_off;  // u8  [n_bytes]            full bytecode
    uint32_t cov_off;    // u8  [n_instr]            coverage bytes
    uint32_t run_off[2]; // u32 [n_instr][2]         straight-line run from each instruction: [0] the run
                         //                          set with the environment pushes, [1] without (MG_K1_RUNENV=0)
    uint32_t fent_off;   // u8  [n_instr]            bit 0: index is a function entry, bit 1: index + 1 is
    uint32_t dec_off;    // u32 [n_instr][2]         kernel 1's pre-decoded words of each instruction (gas;
                         //                          opcode, counts, kind, flags), without the hook bit, which
                         //                          a launch adds; 8-byte aligned, as the run tables are
};

// Per-launch statistics accumulated by the stepping kernel.
struct DevCounters {
    unsigned long long lane_steps;
    unsigned int running, halted, hooked, escaped;
};

#define MG_JRES_NONE 0xffffffffu

// Kernel 1's Keccak result table: one per context, the second level behind the
// per-wave LDS cache.  Direct-mapped, KT_SLOTS entries of KT_ENTRY dwords (128
// bytes): 16 input dwords, 8 hash limbs, the state word at KT_STATE, padding.
// It takes only SHA3 inputs of 64 aligned bytes that are one value in every lane
// of a wave running the SHA3 (keccak(actor . slot): constants of an analysis that
// every wave of every launch hashes again); the kernel fills it and it outlives
// launches.  State: 0 = free, KT_BUSY = claimed (and left so if the claimant never
// finished), otherwise the epoch of the launch that published the entry.  A launch
// uses an entry only when 0 < state < its own epoch, i.e. one that a whole earlier
// launch on the context's stream wrote: the kernel boundary orders those writes,
// so the path needs no fences, and a stale state word can only read as free or as
// the running launch's epoch, both a miss.  Insert-only: nothing is overwritten.
#define KT_SLOTS 64u
#define KT_ENTRY 32u
#define KT_STATE 24u
#define KT_BUSY 0xffffffffu
#define KT_BYTES (KT_SLOTS * KT_ENTRY * 4u)
#define KT_EPOCH_MAX 0xfffffff0u    // launch_step clears the table and restarts the epochs here
