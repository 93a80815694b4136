/*
 * mythgpu.h — C-ABI of libmythgpu.so, the MI355X batched execution core for
 * Mythril's LASER engine.
 *
 * The reference (dellalibera/mythril v0.23.18) is pure Python and has no FFI;
 * its hot path is a set of Python seams.  Each entry point
 * below names the seam it replaces; the Python host layer in mythril_amd/
 * binds them with ctypes (ctypes releases the GIL around every call).
 *
 * Conventions
 *   - every call returns 0 on success or a negative MG_E* code and never throws
 *     across the ABI; the message of the last failure is kept per context and
 *     returned by mg_last_error();
 *   - a 256-bit EVM word is 8 little-endian uint32 limbs (limb 0 = bits 0..31);
 *   - host buffers are plain lane-major arrays (mg_lane_soa); the device keeps
 *     its own lane-interleaved layout and transposes on upload/download;
 *   - one context per GPU, used from one host thread at a time.
 */
#ifndef MYTHGPU_H
#define MYTHGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_ABI_VERSION 15u  /* 2: model tables (arrays, uninterpreted functions)
                               3: per-lane instruction traces + loop bound
                               4: per-lane function-manager records (Keccak, EXP)
                               5: symbolic lanes: expression arena, MG_FORK
                               6: taint lanes: object handles + annotation masks
                               7: symbolic memory bytes, storage chains, symbolic
                                  SHA3 (MG_SYM_SLOAD..CONCAT, MG_REC_SYMKECCAK)
                               8: mg_lanes_download_live; kernel-2 programs keep
                                  the accumulator in operand A (bvrsub, rconcat)
                               9: mg_lanes_upload_live; lane transfers batched
                                  through one pinned DMA per phase; symbolic
                                  calldata copies (MG_SYM_CDBYTE) and a creation's
                                  calldata opcodes (MG_REC_CDSIZE) on symbolic lanes;
                                  symbolic EXP (MG_SYM_BIN 0x0a, MG_REC_SYMEXP)
                              10: MG_LANE_RETDATA (a host CALL left return data:
                                  RETURNDATASIZE / RETURNDATACOPY escape)
                              11: mg_cc_* (native conjunct compiler for kernel 2)
                              12: CALLDATACOPY of a symbolic size / memory offset /
                                  calldata offset on symbolic lanes (MG_SYM_CDBYTEX)
                              13: MLOAD / MSTORE / MSTORE8 at symbolic memory offsets
                                  (MG_SYM_MSTOREK events, MG_SYM_MLOADK reads)
                              14: SHA3 at a symbolic offset (MLOADK ranges), RETURN /
                                  REVERT of a symbolic range (MG_RET_SYMBOLIC),
                                  SELFBALANCE on MG_LANE_SYMBAL lanes, RETURNDATASIZE
                                  on MG_LANE_SYMRDS lanes, RETURNDATACOPY of a
                                  symbolic operand (pops only), BALANCE on
                                  MG_LANE_BALANCE lanes (MG_SYM_BALANCE), symbolic
                                  jump targets (JUMP: VmException, JUMPI: falls
                                  through), SHA3 of a symbolic length (MG_REC_SYMLEN),
                                  GAS / COINBASE / TIMESTAMP / DIFFICULTY on symbolic
                                  lanes (MG_ENV_GAS..MG_ENV_DIFFICULTY), NUMBER /
                                  CHAINID on MG_LANE_SYMBLOCK lanes, LOG0..4 of
                                  symbolic operands (pops only)
                              15: function-entry tracking (mg_lane_soa.fent,
                                  mg_code_fentries): the last JUMP / JUMPI landing
                                  on a dispatcher entry, for active_function_name;
                                  additive: mg_eval_terms, mg_eval_min, mg_lanes_fork,
                                  mg_explore_alloc / mg_explore / mg_explore_download,
                                  mg_explore_upload, mg_explore_check,
                                  mg_explore_check_fn (mg_path_functions) */

/* ------------------------------------------------------------------ errors */
#define MG_OK          0
#define MG_EINVAL     -1   /* bad argument (shape, size, id)                   */
#define MG_EDEVICE    -2   /* HIP runtime failure                               */
#define MG_ENOMEM     -3   /* device or host allocation failed                  */
#define MG_ESTATE     -4   /* call out of order (e.g. step before upload)       */
#define MG_ENOCODE    -5   /* unknown code_id                                   */
#define MG_EUNSUPPORTED -6 /* a constraint the device does not evaluate (mg_cc_compile) */

/* ------------------------------------------------------------ lane status */
/* What ended (or paused) a lane.  Fields pc/sp/msize/gas of a lane that is no
 * longer RUNNING describe the state at the START of the instruction that ended
 * it — the same state the reference puts in `final_states` with track_gas=True
 * (svm.py:331-334 appends the pre-step global_state).                       */
#define MG_RUNNING        0u  /* max_steps reached, still runnable              */
#define MG_HALT_STOP      1u  /* STOP: TransactionEndSignal, world state kept   */
#define MG_HALT_RETURN    2u  /* RETURN: world state kept, ret_offset/ret_len   */
#define MG_HALT_REVERT    3u  /* REVERT: world state discarded                  */
#define MG_HALT_END       4u  /* pc past the instruction list (svm.py:384-389)  */
#define MG_HALT_DROPPED   5u  /* JUMPI true branch to invalid target: no
                                 successor and no exception (instructions.py:1614-1636) */
#define MG_VMEXC          6u  /* VmException; aux = MG_EXC_*                    */
#define MG_HOOK           7u  /* yielded before an opcode set in hook_mask      */
#define MG_ESCAPE         8u  /* needs host semantics; aux = op | reason << 8   */
#define MG_DEPTH          9u  /* strategy depth cutoff (strategy/__init__.py:29) */
#define MG_LOOP_BOUND    10u  /* BoundedLoopsStrategy dropped the state at a JUMPDEST
                                 (bounded_loops.py:119-145); aux = loop count      */

/* ret_len of a symbolic lane's RETURN / REVERT whose offset or length is symbolic
 * (instructions.py:1858-1934): the return data are the reference's fresh
 * "return_data" bytes or a slice at symbolic keys, which the host does not
 * read; LaneBatch.return_data gives None.  (A creation's RETURN of that kind
 * escapes: its return data would be the runtime code.)                     */
#define MG_RET_SYMBOLIC 0xFFFFFFFFu

#define MG_EXC_STACK_UNDERFLOW     1u
#define MG_EXC_STACK_OVERFLOW      2u
#define MG_EXC_INVALID_JUMP        3u
#define MG_EXC_INVALID_INSTRUCTION 4u
#define MG_EXC_OUT_OF_GAS          5u
#define MG_EXC_WRITE_PROTECTION    6u

#define MG_ESC_OPCODE   1u   /* opcode with symbolic or world-state semantics   */
#define MG_ESC_MEMORY   2u   /* memory would grow past the lane's page          */
#define MG_ESC_STORAGE  3u   /* storage slot table full                         */
#define MG_ESC_STACK    4u   /* stack would grow past the lane's stack_cap      */
#define MG_ESC_TRACE    5u   /* instruction trace would grow past trace_cap      */
#define MG_ESC_RECORD   6u   /* function-manager record log would grow past rec_cap */
#define MG_ESC_SYMBOLIC 7u   /* symbolic operand the device has no symbolic semantics for */
#define MG_ESC_ARENA    8u   /* the lane's expression arena / constant table is full */
#define MG_ESC_TAINT    9u   /* the lane's annotation atoms (MG_TAINT_MAX_ATOMS) or object table are full */

/* Function-manager records: what the reference registers with its global
 * function managers while a path runs, logged per lane in execution order so
 * the host can replay the registrations when it materialises the lane.
 * A record is [kind][len][step][result: 8 limbs][payload], in uint32 words;
 * step = the lane's `steps` count before the instruction (its BFS round), so
 * the host can replay registrations of all lanes in the reference's global order.
 *   MG_REC_KECCAK  SHA3 of a concrete, non-empty memory slice
 *                  (keccak_function_manager.create_keccak, keccak_function_manager.py:95-114:
 *                  concrete_hashes[data] = hash).  len = input bytes; result =
 *                  the hash; payload = ceil(len/4) words, input bytes packed
 *                  big-endian (byte 4j+0 in bits 31..24 of word j).
 *   MG_REC_EXP     EXP of concrete operands (exponent_function_manager.py:32-47:
 *                  the path gains the constraint result == Power(base, exponent),
 *                  instructions.py:624-638).  len = 0; result = base**exp mod 2^256;
 *                  payload = base limbs then exponent limbs (16 words).             */
#define MG_REC_KECCAK   1u
#define MG_REC_EXP      2u
/*   MG_REC_ANNOT   a batch-safe annotating hook the device applied (taint lanes,
 *                  mg_taint_program): len = the new atom's index; result = the
 *                  word at stack[-1] before the instruction; payload = stack[-2]
 *                  (8 limbs, 0 when absent), then pc (instruction index) and the
 *                  opcode with MG_TAINT_POST (bit 8) for a post-hook atom, then the
 *                  lane's fent (ABI v15: the hook's active_function_name).  The host
 *                  replays the module's own hook on a state built from it.        */
#define MG_REC_ANNOT    3u
/*   MG_REC_HOOK    a deferred batch-safe hook (MG_TAINT_DEFER): len = n words; result =
 *                  stack[-1]; payload = stack[-2..-n] (8 limbs each), pc, opcode, and
 *                  the lane's fent (the function name the hook sees, ABI v15).    */
#define MG_REC_HOOK     4u
/*   MG_REC_SYMKECCAK  SHA3 of a symbolic input (symbolic lanes): len = input bytes,
 *                  result limbs unused; payload = the MG_SYM_KECCAK node's index.
 *                  The host registers the input with create_keccak in the
 *                  reference's global order (symbolic_inputs).                 */
#define MG_REC_SYMKECCAK 5u
/*   MG_REC_CDSIZE  CODESIZE of a creation transaction on a symbolic lane
 *                  (instructions.py:979-1000): result = the code's size + 0x200, the
 *                  value pushed; the host appends `calldata.size == result` to the
 *                  path's constraints.  len = 0, no payload.                       */
#define MG_REC_CDSIZE   6u
/*   MG_REC_SYMEXP  EXP with a symbolic operand (symbolic lanes, instructions.py:624-638):
 *                  payload = the MG_SYM_BIN node (immediate 0x0a) pushed as the result,
 *                  Power(base, exponent); the host appends exponent_function_manager's
 *                  condition for (base, exponent) to the path.  len = 0.            */
#define MG_REC_SYMEXP   7u
/*   MG_REC_SYMLEN  SHA3 with a symbolic length (symbolic lanes, sha3_, instructions.py:
 *                  1023-1028): the length is taken as 64 and the host appends
 *                  `length == 64` to the path's constraints; len = 64, payload = the
 *                  length's arena node.  Precedes the SHA3's MG_REC_SYMKECCAK.      */
#define MG_REC_SYMLEN   8u
#define MG_REC_HEADER   11u  /* kind, len, step, 8 result limbs                */
#define MG_REC_ANNOT_WORDS (MG_REC_HEADER + 11u)  /* an MG_REC_ANNOT record: stack[-2], pc, opcode, fent */

/* lane flags */
#define MG_LANE_STATIC    1u  /* environment.static (WriteProtection)          */
#define MG_LANE_CREATION  2u  /* ContractCreationTransaction: CODE and CALLDATA ops escape */
#define MG_LANE_HOOK_ACK  4u  /* the host has fired the hooks of the instruction at pc:
                                 the first instruction of the next mg_step call runs
                                 even if its opcode is set in hook_mask; cleared by
                                 the device once that instruction has executed     */
#define MG_LANE_STEP1     8u  /* execute at most one instruction per mg_step call
                                 (the host fires post-hooks on the successor)     */
#define MG_LANE_SYMBOLIC 16u  /* symbolic lane: stepped by the symbolic stepper with
                                 stack tags and an expression arena (mg_sym_alloc) */
#define MG_LANE_SYMCD    32u  /* symbolic calldata (SymbolicCalldata): CALLDATALOAD
                                 and CALLDATASIZE make arena nodes, CALLDATACOPY escapes */
#define MG_LANE_SYMENV_SHIFT 6 /* bit 6 + MG_ENV_k: environment word k is symbolic  */
#define MG_LANE_TAINT  2048u  /* taint lane: stack words are objects with annotation
                                 sets (mg_taint_alloc); stepped by the symbolic stepper */
#define MG_LANE_SYMSTORE 4096u /* symbolic lane whose storage base is the symbolic
                                 Array("Storage{address}") (account.py:26-29), not K(0) */
#define MG_LANE_MEMTAG 8192u  /* symbolic lane whose memory may hold symbolic bytes
                                 (mtag); set by the host or by the device on a write */
#define MG_LANE_RETDATA 16384u /* the path's last_return_data is set (a CALL the host's
                                 escape handler ran): RETURNDATASIZE and RETURNDATACOPY
                                 escape; without it they push 0 / pop only, as the
                                 reference does with last_return_data None
                                 (instructions.py:1314-1370)                       */
#define MG_LANE_SYMBAL 32768u /* symbolic lane whose active account's balance is
                                 symbolic: SELFBALANCE pushes an MG_SYM_ENV node
                                 (w = MG_ENV_SELFBALANCE, instructions.py:968-976) */
#define MG_LANE_SYMRDS 65536u /* symbolic lane whose last_return_data has a symbolic
                                 size (a host CALL's returndatasize variable):
                                 RETURNDATASIZE pushes an MG_SYM_ENV node
                                 (w = MG_ENV_RETURNDATASIZE, instructions.py:1359-1370) */
#define MG_LANE_BALANCE 131072u /* symbolic lane of a LaserEVM with no dynamic loader: BALANCE
                                   pushes an MG_SYM_BALANCE node (the world state's accounts
                                   cannot change inside a device run)                    */
#define MG_LANE_SYMBLOCK 262144u /* symbolic lane whose environment's block_number and chainid are
                                    symbolic: NUMBER / CHAINID push MG_SYM_ENV nodes          */

/* environment words, per lane */
#define MG_ENV_ADDRESS   0
#define MG_ENV_CALLER    1
#define MG_ENV_ORIGIN    2
#define MG_ENV_CALLVALUE 3
#define MG_ENV_GASPRICE  4
#define MG_ENV_WORDS     5
#define MG_ENV_SELFBALANCE 5  /* MG_SYM_ENV immediate only: environment.active_account.balance() */
#define MG_ENV_RETURNDATASIZE 6 /* MG_SYM_ENV immediate only: last_return_data.size */
#define MG_ENV_GAS 7           /* MG_SYM_ENV immediate only: new_bitvec("gas", 256) (gas_, instructions.py:1700-1709) */
#define MG_ENV_COINBASE 8      /* ... new_bitvec("coinbase", 256) (coinbase_, :1386-1393)                      */
#define MG_ENV_TIMESTAMP 9     /* ... new_bitvec("timestamp", 256) (timestamp_, :1396-1403)                    */
#define MG_ENV_DIFFICULTY 10   /* ... new_bitvec("block_difficulty", 256) (difficulty_, :1416-1425)            */
#define MG_ENV_NUMBER 11       /* ... environment.block_number (number_, :1406-1413), on MG_LANE_SYMBLOCK lanes  */
#define MG_ENV_CHAINID 12      /* ... environment.chainid (chainid_, :958-965), on MG_LANE_SYMBLOCK lanes        */

#define MG_STACK_LIMIT 1024u              /* MachineStack.STACK_LIMIT           */
#define MG_MSTATE_GAS_LIMIT 1000000000ull /* GlobalState default gas_limit      */

/* ------------------------------------------------------- host lane layout */
/* Lane-major host image of a batch of concrete EVM paths.  Any pointer may be
 * NULL on download to skip that field; mg_lanes_download_live bounds rows by
 * their count array, so there a row field that is requested (non-NULL, with a
 * non-zero capacity) needs its count: sp for stack, storage_count for storage,
 * msize for memory, trace_len for trace, rec_len for rec (else MG_EINVAL).
 * An upload reads every array (only fent may be NULL).                      */
typedef struct mg_lane_soa {
    uint32_t n;             /* lanes described by the arrays below            */
    uint32_t stack_cap;     /* stack entries per lane in `stack`              */
    uint32_t mem_cap;       /* bytes per lane in `memory` (multiple of 32)    */
    uint32_t calldata_cap;  /* bytes per lane in `calldata`                   */
    uint32_t storage_cap;   /* slots per lane in `storage`                    */
    uint32_t _pad;
    uint32_t *code_id;      /* [n]                                             */
    uint32_t *pc;           /* [n] instruction INDEX (Appendix A #1)          */
    uint32_t *sp;           /* [n] stack depth                                */
    uint32_t *msize;        /* [n] memory size in bytes                       */
    uint32_t *depth;        /* [n] JUMPI depth (mstate.depth)                 */
    uint32_t *status;       /* [n] MG_RUNNING / MG_HALT_* / ...               */
    uint32_t *aux;          /* [n] exception kind / escape op|reason / hook op */
    uint32_t *steps;        /* [n] lane-steps executed (cumulative)           */
    uint32_t *flags;        /* [n] MG_LANE_*                                  */
    uint64_t *gas_min;      /* [n] mstate.min_gas_used                        */
    uint64_t *gas_max;      /* [n] mstate.max_gas_used                        */
    uint64_t *gas_limit;    /* [n] transaction gas_limit                      */
    uint32_t *calldata_len; /* [n]                                             */
    uint8_t  *calldata;     /* [n][calldata_cap]                              */
    uint32_t *env;          /* [n][MG_ENV_WORDS][8]                           */
    uint32_t *stack;        /* [n][stack_cap][8]   slot 0 = bottom            */
    uint8_t  *memory;       /* [n][mem_cap]                                    */
    uint32_t *storage_count;/* [n]                                             */
    uint32_t *storage;      /* [n][storage_cap][16] key limbs 0..7, value 8..15 */
    uint32_t *ret_offset;   /* [n] RETURN/REVERT data offset (low 32 bits)    */
    uint32_t *ret_len;      /* [n] RETURN/REVERT data length (low 32 bits)    */
    /* JumpdestCountAnnotation.trace (bounded_loops.py:14-26): the byte address of
     * every instruction the path has been popped at, when traces are on       */
    uint32_t trace_cap;     /* entries per lane in `trace` (0: no traces)      */
    uint32_t _pad2;
    uint32_t *trace_len;    /* [n]                                             */
    uint32_t *trace;        /* [n][trace_cap]                                  */
    /* function-manager records (MG_REC_*), in execution order                  */
    uint32_t rec_cap;       /* uint32 words per lane in `rec` (0: not recorded) */
    uint32_t _pad3;
    uint32_t *rec_len;      /* [n] words used                                  */
    uint32_t *rec;          /* [n][rec_cap]                                    */
    /* LaserEVM._new_node_state (svm.py:575-637): after every JUMP / JUMPI the
     * successor's instruction address switches environment.active_function_name
     * when it is a dispatcher entry (Disassembly.address_to_function_name,
     * disassembly.py:36-56) or address 0 ("fallback").  The device keeps the
     * instruction INDEX of the last such landing since the upload, or
     * MG_FENT_NONE; the host maps it to the name.  NULL: uploads MG_FENT_NONE,
     * downloads nothing (ABI <= 14 callers).                                  */
    uint32_t *fent;         /* [n]                                             */
} mg_lane_soa;
#define MG_FENT_NONE 0xffffffffu

/* Per-call statistics of mg_step. */
typedef struct mg_step_stats {
    uint64_t lane_steps;    /* instructions executed by all lanes in the call */
    uint32_t running;       /* lanes still MG_RUNNING after the call          */
    uint32_t halted;        /* lanes in a terminal status                     */
    uint32_t hooked;        /* lanes in MG_HOOK                               */
    uint32_t escaped;       /* lanes in MG_ESCAPE                             */
    float    kernel_ms;     /* device time of the stepping kernel(s)          */
    uint32_t launches;      /* kernel launches issued                         */
} mg_step_stats;

/* Batch configuration, fixed at mg_lanes_alloc. */
typedef struct mg_batch_cfg {
    uint32_t n_lanes;
    uint32_t stack_cap;     /* <= MG_STACK_LIMIT                              */
    uint32_t mem_cap;       /* bytes, multiple of 32                           */
    uint32_t calldata_cap;  /* bytes                                           */
    uint32_t storage_cap;   /* slots                                           */
    uint32_t coverage;      /* 1: record the per-code coverage bitmap         */
    uint32_t trace_cap;     /* instruction-trace entries per lane (0: none)   */
    uint32_t rec_cap;       /* function-manager record words per lane (0: none) */
} mg_batch_cfg;

typedef struct mg_ctx mg_ctx;

/* ---------------------------------------------------------- symbolic lanes
 * A symbolic lane keeps every stack word's value plus a tag: 0 = concrete,
 * else 1 + the index of the arena node that defines it.  Arena node = 4 u32:
 *   x = kind | width << 8 (width 1: a Bool, 256: a bit-vector),
 *   y, z = operand refs (MG_SYM_CONST | k: entry k of the lane's constant
 *          table; else a node index), w = immediate (EVM opcode / env word).
 * Kinds (the host builds the reference's expression for each, see
 * mythril_amd/laser/symbolic.py): */
#define MG_SYM_CDLOAD 1u  /* calldata.get_word_at(y) (state/calldata.py:214-262)  */
#define MG_SYM_CDSIZE 2u  /* calldata.calldatasize                               */
#define MG_SYM_ENV    3u  /* environment word w (MG_ENV_*)                       */
#define MG_SYM_BIN    4u  /* binary EVM opcode w on (y = first pop, z = second)  */
#define MG_SYM_UN     5u  /* unary EVM opcode w (ISZERO, NOT) on y               */
#define MG_SYM_SLOAD  6u  /* simplify(Select(store chain after its first z entries, y))
                             (account.py:43-75, instructions.py:1496-1506)        */
#define MG_SYM_KECCAK 7u  /* keccak256_w(y): create_keccak of a symbolic input of w bits
                             (keccak_function_manager.py:95-114, instructions.py:1013-1051) */
#define MG_SYM_EXTRACT 8u /* Extract(w >> 16, w & 0xffff, y) of a node's word      */
#define MG_SYM_CONCAT 9u  /* Concat(y, z), widths w & 0xffff and w >> 16: the parts of
                             a memory read, simplify(Concat(bytes)) (memory.py:56-82) */
#define MG_SYM_TERM  10u  /* an opaque term of the host's expression layer, index w in
                             the host's term table (anything a handler or the caller
                             built); compared by identity                          */
#define MG_SYM_CDBYTE 12u /* calldata[w]: one 8-bit byte of the calldata, If(w < size,
                             calldata_array[w], 0) (state/calldata.py:253-262), as
                             _calldata_copy_helper writes it (instructions.py:807-875) */
#define MG_SYM_CDBYTEX 13u /* calldata[simplify(y + w)]: byte w of a CALLDATACOPY from a
                              symbolic calldata offset y (instructions.py:816-860; a
                              symbolic size copies 320 bytes, call.py:33)           */
#define MG_SYM_MSTOREK 14u /* an event, not a term: a write at the symbolic memory offset y
                              of value ref z -- w = 1: MSTORE (write_word_at), 2: MSTORE8
                              (the value's low byte), 3: one byte (a host-encoded key).  The
                              lane's events in arena order are its byte map at symbolic keys
                              (memory.py:117-203, keys simplify(index))                    */
#define MG_SYM_MLOADK 15u  /* a read at the symbolic offset y over the byte map the events
                              before this node build: w = 0, memory.get_word_at(y) (MLOAD,
                              instructions.py:1439-1451); w = n > 0, simplify(Concat(memory[y :
                              y + n])) (the data of a SHA3, instructions.py:1014-1051)     */
#define MG_SYM_BALANCE 16u /* BALANCE of the address ref y (balance_, instructions.py:907-931,
                              no dynamic loader): the account's balance() when y is a known
                              concrete address, else the If chain over the world state's
                              accounts; on MG_LANE_BALANCE lanes                           */
#define MG_SYM_CONST  0x80000000u
#define MG_FORK      11u  /* status: JUMPI on a symbolic condition; the lane holds
                             the state at the start of the JUMPI (host forks)    */

/* Host image of the symbolic planes of lanes [first, first + n), lane-major.
 * Every pointer is required, on upload and on download (none may be NULL).
 * Memory bytes and storage entries carry tags too (ABI v7): a memory byte tag is
 * 0 (the byte in `memory` is the value) or 1 + (node << 5 | j): byte j (0 = most
 * significant) of that node's word, i.e. Extract(255 - 8j, 248 - 8j, word) as
 * write_word_at stores it (memory.py:84-115).  In a symbolic lane the storage
 * table is the reference's store chain, one entry per SSTORE in order (over K(0),
 * or the symbolic Array with MG_LANE_SYMSTORE); an entry's key / value tag is 0
 * (the limbs are the value) or 1 + node. */
typedef struct mg_sym_soa {
    uint32_t n, stack_cap, node_cap, const_cap;
    uint32_t *stag;         /* [n][stack_cap]                                 */
    uint32_t *node;         /* [n][node_cap][4]                               */
    uint32_t *cval;         /* [n][const_cap][8] little-endian limbs          */
    uint32_t *n_nodes;      /* [n]                                            */
    uint32_t *n_consts;     /* [n]                                            */
    uint32_t mem_cap, storage_cap;   /* the lane image's capacities               */
    uint32_t *mtag;         /* [n][mem_cap] memory byte tags                  */
    uint32_t *sttag;        /* [n][storage_cap][2] storage entry (key, value) tags */
} mg_sym_soa;

/* Symbolic planes for the current batch (after mg_lanes_alloc; freed with it).
 * Lanes flagged MG_LANE_SYMBOLIC are stepped by the symbolic stepper in the same
 * mg_step / mg_step_until call, right after the concrete stepper. */
int         mg_sym_alloc(mg_ctx *ctx, uint32_t node_cap, uint32_t const_cap);
int         mg_sym_upload(mg_ctx *ctx, const mg_sym_soa *host, uint32_t first, uint32_t n);
int         mg_sym_download(mg_ctx *ctx, mg_sym_soa *host, uint32_t first, uint32_t n);

/* ------------------------------------------------------------ taint lanes
 * The reference's stack words are Python objects carrying a mutable set of
 * annotations (laser/smt/expression.py:10-57): ALU results take the union of
 * their operands' sets (bitvec.py:63-136), DUP pushes the SAME object
 * (instructions.py:330) so a later annotate() on it shows on every copy, the
 * environment words are one object each (instructions.py:895-1060), and concrete
 * memory / storage round trips drop them (memory.py:84-115, account.py:43-87).
 * A taint lane (MG_LANE_TAINT) reproduces that on the device: every stack slot
 * holds an object handle (0: an object no other slot shares and that has no
 * annotations; 1..5: the environment words MG_ENV_k + 1; 6: the symbolic
 * calldata size; >= 7: the lane's object table), and every object an annotation
 * mask over the lane's atoms (<= 64; the host maps atom k to annotation objects).
 *
 * Batch-safe hooks (mythril_amd/laser/taint.py) become per-opcode actions the
 * device applies instead of yielding to the host, and log an MG_REC_ANNOT record
 * per new atom.  No action applies to an instruction that has fewer stack
 * words than its opcode requires: it raises before any hook runs
 * (svm.py:391-405).  Action word per opcode byte (mg_taint_program): */
#define MG_TAINT_PRE_SHIFT   0   /* bits 0..3: operand k + 1 of a pre-hook that annotates stack[-1-k] */
#define MG_TAINT_POST       16u  /* a post-hook annotates the pushed word                     */
#define MG_TAINT_EXPCOND    32u  /* skip the pre-annotation when stack[-2] == 0 or stack[-1] < 2
                                    (integer.py:161-166)                                        */
#define MG_TAINT_YCLASS     64u  /* this action's atoms join the lane's yield class            */
#define MG_TAINT_SINK_SHIFT  8   /* bits 8..11: operand k + 1 whose set a pre-hook adds to the
                                    state annotation (the lane's sink mask)                    */
#define MG_TAINT_YIELD_SHIFT 12  /* bits 12..15: operand k + 1: yield (MG_HOOK) only when that
                                    word carries an atom of the yield class                   */
#define MG_TAINT_DEFER_SHIFT 16  /* bits 16..19: 1..3: a pre-hook replayed later from a record of
                                    stack[-1..-n] (MG_REC_HOOK); it reads only those words     */
#define MG_TAINT_IFSYM_SHIFT 20  /* bits 20..23: operand k + 1: a pre-hook with work only when that
                                    word is symbolic (yield then)                              */
#define MG_TAINT_IFLANE     (1u << 24)  /* yield when the lane's tflags bit 1 is set (a state
                                    annotation the host found at pack)                          */
#define MG_TAINT_FIELD_BITS  4   /* width of each operand field above (PRE, SINK, YIELD, DEFER, IFSYM) */
#define MG_TAINT_FIELD(action, shift) (((action) >> (shift)) & ((1u << MG_TAINT_FIELD_BITS) - 1u))
#define MG_TAINT_CDSIZE      6u  /* handle of the symbolic calldata-size object                */
#define MG_TAINT_OBJ0        7u  /* first object-table handle                                  */
#define MG_TAINT_MAX_ATOMS  64u  /* atoms per lane: one bit each of an annotation mask         */

/* Host image of the taint planes of lanes [first, first + n), lane-major.
 * Every pointer is required, on upload and on download (none may be NULL). */
typedef struct mg_taint_soa {
    uint32_t n, stack_cap, obj_cap, _pad;
    uint32_t *sobj;         /* [n][stack_cap] object handle per stack slot      */
    uint64_t *omask;        /* [n][obj_cap]   annotation mask per object         */
    uint32_t *n_obj;        /* [n] object handles in use (>= MG_TAINT_OBJ0)     */
    uint32_t *n_fixed;      /* [n] handles below this are the host's objects: the
                               device's handle compaction never renumbers them  */
    uint32_t *n_atoms;      /* [n] atoms in use (<= 64)                          */
    uint64_t *sink;         /* [n] atoms the sink hooks collected                */
    uint64_t *ymask;        /* [n] atoms of the yield class                      */
    uint32_t *tflags;       /* [n] bit 0: a sink hook ran; bit 1: MG_TAINT_IFLANE yields */
} mg_taint_soa;

/* Taint planes for the current batch (after mg_lanes_alloc; freed with it) and
 * the per-opcode action table (256 words; zeros = no batch-safe hooks). */
int         mg_taint_alloc(mg_ctx *ctx, uint32_t obj_cap);
int         mg_taint_program(mg_ctx *ctx, const uint32_t actions[256]);
/* Per instruction of a code (n = its instruction count): 1 = a taint lane stops
 * there with MG_HOOK instead of applying the opcode's actions, 2 = it applies
 * none (addresses in modules' issue caches, where DetectionModule.execute returns
 * early, base.py:79-86: 2 when every module on the opcode has it cached). */
int         mg_taint_force(mg_ctx *ctx, uint32_t code_id, const uint8_t *flags, uint32_t n);
int         mg_taint_upload(mg_ctx *ctx, const mg_taint_soa *host, uint32_t first, uint32_t n);
int         mg_taint_download(mg_ctx *ctx, mg_taint_soa *host, uint32_t first, uint32_t n);

/* ------------------------------------------------------------- lifecycle */
int         mg_abi_version(void);
int         mg_open(int device, mg_ctx **out);
void        mg_close(mg_ctx *ctx);
const char *mg_last_error(mg_ctx *ctx);
/* Opcode table the device uses (support/opcodes.py:16-144 + instruction_data.py:
 * 51-56): gas (min,max) and required stack items for a byte, or -1 if the
 * byte disassembles to INVALID (asm.py:126-131).                            */
int         mg_opcode_info(uint32_t byte, uint32_t *gas_min, uint32_t *gas_max,
                           uint32_t *stack_req);

/* ------------------------------------------------------------------ code */
/* Replaces Disassembly(code) (disassembly.py:9-56, asm.py:99-148) +
 * util.get_instruction_index (util.py:45-59): builds the instruction table
 * (pc = index), push immediates, the ">="-jump-resolve table and keeps the
 * full bytecode for CODECOPY/CODESIZE.                                        */
int         mg_load_code(mg_ctx *ctx, const uint8_t *code, size_t n, uint32_t *code_id);
/* Number of instructions of a loaded code (len(instruction_list)).          */
int         mg_code_info(mg_ctx *ctx, uint32_t code_id, uint32_t *n_instr);
/* The device's function-entry flags of a loaded code, one byte per instruction
 * (n = its instruction count): bit 0 = a JUMP / JUMPI landing on this index
 * switches active_function_name (an entry of the PUSH1..4 EQ PUSHn dispatcher
 * pattern, asm.py:66-94 + disassembly.py:36-56 / 64-114, or index 0 =
 * address 0), bit 1 = the same for the next index (JUMPI fall-through).      */
int         mg_code_fentries(mg_ctx *ctx, uint32_t code_id, uint8_t *out, uint32_t n);
/* The device's instruction table of a loaded code (n = its instruction count):
 * opcode byte per index (0xfe for bytes asm.py:126-131 disassembles to INVALID)
 * and the byte address of each instruction -- Disassembly.instruction_list
 * without the arguments (they are the code's bytes after each PUSH).          */
int         mg_code_table(mg_ctx *ctx, uint32_t code_id, uint8_t *ops, uint32_t *addrs, uint32_t n);

/* ----------------------------------------------------------------- lanes */
int         mg_lanes_alloc(mg_ctx *ctx, const mg_batch_cfg *cfg);
/* Upload lanes [first, first+n) from host (host->n must equal n).  The
 * upload also becomes the batch's resident initial image (see mg_lanes_reset).
 * The scalars, calldata and the environment words go whole (up to the host's
 * calldata_cap); rows go only below the range's largest host count -- stack
 * below the largest sp, memory below the largest msize, storage below the
 * largest storage_count, trace / records below the largest trace_len /
 * rec_len -- and device rows above those bounds, like every lane outside the
 * range, keep their contents (no step reads them before writing them).  A host
 * trace_cap / rec_cap of 0 zeroes the range's trace_len / rec_len.            */
int         mg_lanes_upload(mg_ctx *ctx, const mg_lane_soa *host, uint32_t first, uint32_t n);
int         mg_lanes_download(mg_ctx *ctx, mg_lane_soa *host, uint32_t first, uint32_t n);
/* mg_lanes_download of what the lanes can have changed, for a host image that
 * was uploaded from the same buffers: the scalars, then each lane's stack rows
 * below the largest sp of the range, memory below the largest msize, storage
 * entries below the largest storage_count, records below the largest rec_len
 * and trace entries below the largest trace_len (the device's counts, clipped
 * to the host's capacities).  calldata and the environment
 * words (never written by a step) and everything above those bounds keep the
 * host's contents.  A requested row field whose count array is NULL is refused
 * with MG_EINVAL (the error names the array) before anything is launched.  The
 * batched LaserEVM's per-launch copy-back
 * (svm.py:293-337 drain) -- a full download moves every lane's whole stack.  */
int         mg_lanes_download_live(mg_ctx *ctx, mg_lane_soa *host, uint32_t first, uint32_t n);
/* The same transfer as mg_lanes_upload (every upload is bounded by the range's
 * largest counts since ABI v9's round 4; the name is kept for callers that say
 * what they rely on): the scalars, calldata and environment
 * words whole, each lane's stack rows below the largest sp of the range,
 * memory below the largest msize (a step zero-fills memory it extends),
 * storage entries below the largest storage_count, trace entries below the
 * largest trace_len and records below the largest rec_len; device rows above
 * those bounds keep their contents.  The batched LaserEVM's per-launch upload
 * of the lanes its host hooks touched (svm.py:369-491 resume).               */
int         mg_lanes_upload_live(mg_ctx *ctx, const mg_lane_soa *host, uint32_t first, uint32_t n);
/* Re-initialise every lane from the resident initial image on the device
 * (no host traffic): pc, sp, msize, gas, status, storage, steps.            */
int         mg_lanes_reset(mg_ctx *ctx);

/* The fork of a JUMPI on a symbolic condition (jumpi_, instructions.py:1558-1636:
 * two copies of the state, one per branch, each with one more path constraint)
 * as a lane-image operation on the device: nothing crosses PCIe but the index
 * arrays below and the two result arrays.
 *
 * Fork i makes up to two successors of lane src[i]: the fall-through in lane
 * dst_fall[i] and the jump in lane dst_jump[i].  A source is forkable when its
 * status is MG_FORK, its flags have MG_LANE_SYMBOLIC and not MG_LANE_TAINT,
 * sp >= 2, stag[sp-1] == 0 (a concrete target), stag[sp-2] != 0 (a symbolic
 * condition) and its pc is an instruction of its code; otherwise made[i] =
 * MG_FORK_BAD_SRC, cond[i] = 0 and no lane is written (a normal answer: the host
 * does not know device statuses without a download).
 *
 * cond[i] = the source's stag[sp-2], 1 + the arena node of the condition.  Both
 * successors keep that node at the same index of their copied arena; the host
 * appends `condition` to the jump's constraints and Not(condition) to the
 * fall-through's, as jumpi_ does.
 *
 * A successor is what the stepper's concrete JUMPI leaves when that side is
 * taken: sp - 2, depth + 1, gas_min / gas_max + 10 (by hand, no out-of-gas
 * check), steps + 1, status MG_RUNNING, aux 0, MG_LANE_HOOK_ACK cleared and the
 * other flags kept.  Fall-through: pc + 1, and fent = pc + 1 when bit 1 of the
 * JUMPI's function-entry flags is set.  Jump: idx = the ">="-resolve of the target when
 * it fits 32 bits and is below the table's size; valid when the instruction at
 * idx is a JUMPDEST; then pc = idx, and fent = idx when bit 0 of idx's flags is
 * set.  An invalid target makes no jump lane (dst_jump[i] is untouched and
 * MG_FORK_MADE_JUMP stays clear; the reference returns only the fall-through).
 * Everything else is the source's, copied below its live bounds only: stack rows
 * and stag below sp - 2, memory and mtag below msize, storage entries and sttag
 * below storage_count, arena nodes below n_nodes, constants below n_consts,
 * records below rec_len, trace below trace_len (the JUMPI is already in it),
 * calldata and the environment words whole, and every remaining scalar (the
 * Keccak / EXP event counts included).  Destination rows above those bounds and
 * every lane not named keep their contents, as after an upload.  With coverage
 * on, the JUMPI's byte is set when a successor is made.  The resident reset
 * image is not touched: mg_lanes_reset and mg_run_batches still restart from
 * the last upload.
 *
 * Checked on the host before any launch (MG_ESTATE: no batch, no upload or no
 * symbolic planes; else MG_EINVAL; the message names the offending index; the
 * device image is unchanged): every lane index is below n_lanes, all src are
 * distinct, all destinations other than MG_FORK_NONE are distinct from one
 * another and from every src except dst_fall[i] == src[i] (the source becomes
 * its own fall-through in place), dst_jump[i] != src[i], made and cond are
 * non-NULL when n > 0.  n == 0 succeeds and does nothing.  The number of
 * launches and copies does not depend on n.                                   */
#define MG_FORK_NONE      0xffffffffu  /* dst: do not make this successor          */
#define MG_FORK_MADE_FALL 1u           /* made[]: the fall-through lane was written */
#define MG_FORK_MADE_JUMP 2u           /* made[]: the jump lane was written         */
#define MG_FORK_BAD_SRC   0x80000000u  /* made[]: src is not a forkable lane; nothing written */
typedef struct mg_fork_batch {
    uint32_t n, _pad;
    const uint32_t *src;       /* [n] lanes stopped with MG_FORK                      */
    const uint32_t *dst_fall;  /* [n] lane for the fall-through successor, MG_FORK_NONE,
                                      or src[i] itself (the parent becomes it in place) */
    const uint32_t *dst_jump;  /* [n] lane for the jump successor, or MG_FORK_NONE     */
} mg_fork_batch;
int         mg_lanes_fork(mg_ctx *ctx, const mg_fork_batch *forks,
                          uint32_t *made /* [n] */, uint32_t *cond /* [n] */, float *kernel_ms);

/* The step-and-fork loop on the device (the drain of svm.py:293-337 with jumpi_,
 * instructions.py:1558-1636, as its only fork): up to max_rounds rounds, each one
 * stepping launch as mg_step makes it, then the fork of every lane that stopped at
 * a symbolic JUMPI, planned where the statuses are.  The host reads one small
 * counter block per round (one stream synchronisation) and uploads nothing after
 * the free list; the numbers of launches and copies per round do not depend on the
 * number of forks.
 *
 * mg_explore_alloc (after mg_sym_alloc, once per batch; freed with the lanes)
 * adds three per-lane planes.  path: up to path_cap entries per lane, entry =
 * cond_tag << 1 | side, where cond_tag is mg_lanes_fork's cond[] value (1 + the
 * arena node of the JUMPI's condition, which every descendant keeps at that index
 * of its copied arena) and side is 1 for the jump and 0 for the fall-through.
 * path_len: the number of entries.  root: the lane's lineage.  mg_explore starts
 * (on the device) by setting root[l] = l and path_len[l] = 0 for every lane, so a
 * lane that comes back has root = the lane its ancestor held when the call began
 * and path = the branches taken since, oldest first; the host appends `condition`
 * for a side-1 entry and Not(condition) for a side-0 entry, as jumpi_ does.
 *
 * The plan of a round.  A lane is a source under mg_lanes_fork's test, unchanged
 * (status MG_FORK, MG_LANE_SYMBOLIC and not MG_LANE_TAINT, 2 <= sp <= stack_cap, a
 * concrete target, a symbolic condition, pc inside its code), and when it is not
 * in the unused part of the free list.  Taint lanes and lanes with a symbolic
 * target are no sources: they stay MG_FORK and are counted nowhere.  A source with
 * path_len == path_cap is left untouched, still MG_FORK, and counts in path_full.
 * The fall-through is always made in place (dst_fall == src).  A source whose
 * target is no JUMPDEST forks in place only and takes no free lane (the reference
 * returns only the fall-through).  The sources with a valid target are ranked in
 * ascending lane order; number r of the round takes free_lanes[used + r] as its
 * jump lane, `used` being the entries earlier rounds of this call took.  When the
 * list runs short the lowest lanes win; the others are left wholly untouched, still
 * MG_FORK, and count in starved: the host forks them by mg_lanes_fork.  n_free == 0
 * is allowed (every fork with a valid target is starved).  The successors are
 * exactly mg_lanes_fork's for (src, dst_fall = src, dst_jump = that free lane or
 * MG_FORK_NONE): the same kernels make them, so coverage, the loop-bound trace,
 * records and the resident reset image behave as stated there.  Then the jump
 * child takes the source's root and path plus a side-1 entry, and the source gains
 * the side-0 entry.
 *
 * Which lanes are free is the caller's statement: a free lane's contents are
 * overwritten when it is handed out (below its source's live bounds, as in
 * mg_lanes_fork), whatever its status was; it is stepped like any lane until then.
 * Entries free_lanes[free_used ...] were not used.
 *
 * The loop ends after a round that planned no fork and found no lane MG_RUNNING,
 * or after max_rounds rounds.  Lanes that forked in the last round are MG_RUNNING
 * on return.  stats: rounds run; forks made; made_jump = jump lanes written =
 * free lanes used in all (free_used); starved and path_full summed over the rounds
 * (a lane left in place counts again each round); running = lanes MG_RUNNING on
 * return; lane_steps and kernel_ms (first launch to last) over the whole call.
 *
 * Checked on the host before any launch (the device image is unchanged):
 * MG_ESTATE without a batch, an upload, symbolic planes or explore planes;
 * MG_EINVAL when max_rounds == 0 (the loop is bounded by its argument), when
 * free_lanes is NULL with n_free > 0, or when free_lanes is not strictly ascending
 * with every entry below n_lanes (the message names the index).
 *
 * mg_explore_download: lanes [first, first + n); path is lane-major on the host,
 * [n][path_cap] (lane i's entries are path[i * path_cap ...]), entries at and
 * above path_len[i] are 0.                                                      */
int         mg_explore_alloc(mg_ctx *ctx, uint32_t path_cap);
typedef struct mg_explore_stats {
    uint32_t rounds, forks, made_jump, starved, path_full, free_used, running, _pad;
    uint64_t lane_steps;
    float    kernel_ms, _padf;
} mg_explore_stats;
int         mg_explore(mg_ctx *ctx, const uint64_t hook_mask[4], uint32_t max_steps,
                       uint32_t max_depth, uint32_t max_rounds, const uint32_t *free_lanes,
                       uint32_t n_free, mg_explore_stats *stats);
int         mg_explore_download(mg_ctx *ctx, uint32_t *path /* [n][path_cap] */,
                                uint32_t *path_len /* [n] */, uint32_t *root /* [n] */,
                                uint32_t first, uint32_t n);
/* The inverse of mg_explore_download, for a caller that keeps paths of its own
 * (a host-made fork, a test's hand-written image): lanes [first, first + n) take
 * path (lane-major, [n][path_cap]; entries at and above path_len[i] are not
 * read), path_len and root.  MG_ESTATE without explore planes; MG_EINVAL, with
 * nothing written, for a range outside the batch, a NULL array with n > 0 or a
 * path_len above path_cap.  root is data: mg_explore_check answers a root outside
 * the batch with MG_PATH_UNKNOWN.  The next mg_explore restarts every lane's path. */
int         mg_explore_upload(mg_ctx *ctx, const uint32_t *path /* [n][path_cap] */,
                              const uint32_t *path_len /* [n] */, const uint32_t *root /* [n] */,
                              uint32_t first, uint32_t n);
/* mg_explore with the paths kept: the same arguments, plan, rounds, statistics and
 * host-side checks, but root, path_len and path stay as the last mg_explore,
 * mg_explore_resume or mg_explore_upload left them; only the free marks are cleared
 * and set again from this call's list.  A lane handed out from the list takes its
 * source's root and path, as any free lane does, whatever path it held before.  A
 * lane that is MG_FORK when the call starts (a starved one) is planned in the
 * first round.  With mg_harvest_select / mg_harvest_download below this is the
 * loop "explore, take out what finished, put those lanes into the free list,
 * explore again" with no path lost and no whole-batch download.               */
int         mg_explore_resume(mg_ctx *ctx, const uint64_t hook_mask[4], uint32_t max_steps,
                              uint32_t max_depth, uint32_t max_rounds, const uint32_t *free_lanes,
                              uint32_t n_free, mg_explore_stats *stats);

/* Finished lanes, chosen where the statuses are and fetched in one transfer.
 *
 * mg_harvest_select.  Lane l < n_lanes matches when status[l] < 32, bit status[l]
 * of status_mask is set and l is not in skip (a lane that was never uploaded holds
 * 0xffffffff and never matches).  skip is the caller's free list -- the lanes whose
 * contents it has already taken or never filled --, strictly ascending, every
 * entry below n_lanes.  The matching lanes are ranked in ascending lane order and
 * the first min(matched, max_lanes) are selected (max_lanes above n_lanes is
 * clipped); their indices stay on the device as an ascending list.  info: n,
 * matched, and the largest sp, msize, storage_count, trace_len, rec_len, n_nodes,
 * n_consts and path_len among the SELECTED lanes (0 when none is selected or the
 * batch has no such plane: trace_cap / rec_cap of 0, no symbolic planes, no explore
 * planes); kernel_ms from the first kernel to the last.  status_mask == 0 and
 * max_lanes == 0 are valid and select nothing.  The call uploads nothing but skip,
 * reads one small block back under one stream synchronisation, and its numbers of
 * launches and copies depend on none of n_lanes, matched and n; it writes nothing
 * of the lane image.  MG_HARVEST_BLOCKS (1..1024, default 1024, read per call) caps
 * the number of blocks that scan the statuses; MG_EXPLORE_BLOCKS (the same range,
 * default and reading) caps those of mg_explore's and mg_explore_resume's plan.
 * Neither changes a result.
 * Checked on the host before any launch: MG_ESTATE without a batch or an upload;
 * MG_EINVAL for a NULL info, a NULL skip with n_skip > 0, or a skip that is not
 * strictly ascending with every entry below n_lanes (the message names the index).
 *
 * mg_harvest_download.  Row i of every host array is device lane lanes[i] of the
 * last mg_harvest_select (host->n and, when given, sym->n must equal its info.n).
 * The scalars, fent (when host->fent is given), calldata and the environment words
 * go whole, as in mg_lanes_download; rows go below the selection's largest count:
 * stack and stag below info.sp, memory and mtag below info.msize, storage and
 * sttag below info.storage_count, trace / records below info.trace_len /
 * info.rec_len (trace_len / rec_len themselves when the host's trace_cap / rec_cap
 * is not 0), arena nodes below info.n_nodes, constants below info.n_consts; every
 * bound is clipped to the host image's capacity, which may be below the batch's,
 * and host cells at and above a bound keep their contents.  A NULL pointer in host
 * skips that field.  sym may be NULL; path, path_len and root are all NULL or all
 * given; path is [n][path_cap] as in mg_explore_download, entries at and above a
 * lane's path_len are 0.  Taint planes are not part of the call.  Everything
 * crosses PCIe in one copy under one stream synchronisation, whatever n is.
 * The selection is dropped by mg_lanes_alloc, mg_sym_alloc and mg_explore_alloc;
 * without one (also before the first select) the call answers MG_ESTATE.  It is
 * not dropped by a step: a download after the image was stepped returns the
 * current image of the listed lanes under the select-time bounds, and still reads
 * inside the planes because every bound is at most a capacity.  MG_EINVAL, with
 * nothing written: host->n (or sym->n) != info.n, capacities above the batch's,
 * path without explore planes, sym without symbolic planes, path / path_len / root
 * not given together.  After a selection of n == 0 the call succeeds and does
 * nothing.                                                                       */
typedef struct mg_harvest_info {
    uint32_t n;        /* lanes selected, <= max_lanes                                   */
    uint32_t matched;  /* lanes that matched; matched - n are left (the lowest lanes win) */
    uint32_t sp, msize, storage_count, trace_len, rec_len,   /* largest count among the  */
             n_nodes, n_consts, path_len;                    /* SELECTED lanes (0 if none
                                                                or the plane is absent)  */
    float    kernel_ms; uint32_t _pad;
} mg_harvest_info;
int         mg_harvest_select(mg_ctx *ctx, uint32_t status_mask, const uint32_t *skip, uint32_t n_skip,
                              uint32_t max_lanes, mg_harvest_info *info);
int         mg_harvest_download(mg_ctx *ctx, uint32_t *lanes /* [n] */, mg_lane_soa *host /* host->n == n */,
                                mg_sym_soa *sym /* or NULL */, uint32_t *path /* [n][path_cap] or NULL */,
                                uint32_t *path_len, uint32_t *root /* both NULL iff path is NULL */);
/* mg_harvest_upload, the inverse of mg_harvest_download: lanes the host has resolved
 * (escapes, hooks) go back into a running batch by list.  Row i of every host array
 * goes to device lane lanes[i], n = host->n rows.  lanes is strictly ascending with
 * every entry below n_lanes; lanes == NULL means the resident list of the last
 * mg_harvest_select ("take out, resolve, put back where it was": no list crosses
 * PCIe), MG_ESTATE without a selection, MG_EINVAL when host->n != its info.n.
 * What is written.  The scalars of mg_lanes_upload, whole; fent is the host's, or
 * 0xffffffff when host->fent is NULL; trace_len / rec_len are the host's, or 0 when
 * the host's trace_cap / rec_cap is 0; sha3_count and exp_count are 0: a planted lane
 * is what mg_lanes_upload of a range would leave.  calldata (up to the host's
 * calldata_cap) and the environment words go whole.  Rows go below the LARGEST COUNT
 * AMONG THE n HOST ROWS, clipped to the host capacities: stack below the largest sp,
 * memory below the largest msize, storage below the largest storage_count, trace and
 * records below the largest trace_len / rec_len.  With sym (sym->n == n): n_nodes and
 * n_consts, node below the largest n_nodes, cval below the largest n_consts, stag
 * below the largest sp, mtag below the largest msize, sttag below the largest
 * storage_count -- the live extent mg_harvest_download and the device fork use, not
 * the full-capacity tag planes of mg_sym_upload.  With path (path, path_len and root
 * all given): path_len, root, and path rows below the largest path_len of the call;
 * entries at and above a lane's own path_len arrive as 0 (the host's are not read).
 * What is not written: unlisted lanes; cells at and above a bound; the resident
 * reset image (a later mg_lanes_reset gives a planted lane the pc, depth, status,
 * aux, steps, gas and storage the image holds for that lane, under the planted
 * code_id, flags, inputs and gas limit); coverage; the explorer's free marks; the
 * resident selection; the symbolic planes when sym is NULL and the path planes when
 * path is NULL.  Taint planes are not part of the call.
 * Every check runs on the host before any copy or launch, and a refused call leaves
 * the image as it was.  MG_ESTATE: no batch, or no earlier mg_lanes_upload.
 * MG_EINVAL: a NULL host; a list that is not strictly ascending below n_lanes (the
 * message names the index); host capacities above the batch's; sym->n != n; sym
 * without symbolic planes; path without explore planes; path / path_len / root not
 * given together; a row whose sp, msize, calldata_len, storage_count, trace_len,
 * rec_len, n_nodes or n_consts is above its host capacity, whose msize is not a
 * multiple of 32 or whose path_len is above path_cap.  MG_ENOCODE: a row with an
 * unknown code_id.  Row messages name the device lane (the row, for the resident
 * list).  Accepted code ids count as used for the stepping kernel's code plan.
 * n == 0 succeeds and does nothing.
 * Cost: one H2D copy (list, scalars and rows in one stage), one stream
 * synchronisation, and numbers of launches and copies that depend on the fields
 * present, never on n or on how the list is spread over the batch.              */
int         mg_harvest_upload(mg_ctx *ctx, const uint32_t *lanes /* [n], or NULL */,
                              const mg_lane_soa *host /* n = host->n */, const mg_sym_soa *sym /* or NULL */,
                              const uint32_t *path /* [n][path_cap] or NULL */, const uint32_t *path_len,
                              const uint32_t *root /* both NULL iff path is NULL */);

/* The fork filter's question, "does any cached model satisfy this lane's path"
 * (svm.py:319-326 -> ModelCache.check_quick_sat, support_utils.py:60-68), answered
 * where the arena is: every path entry of a lane is evaluated straight from the
 * lane's arena under every candidate model, with no download, decode or flatten.
 * The verdict has mg_eval_bits' meaning; the host decodes and flattens only the
 * lanes no candidate satisfies or whose path the device cannot evaluate.
 *
 * It needs mg_sym_alloc and mg_explore_alloc (MG_ESTATE otherwise) and reads the
 * device image as the last mg_explore (or mg_explore_upload) left it: path,
 * path_len, root, the arena, the constants, the storage chain and its tags.  It
 * writes nothing of the image.  For lane l in [first, first + n) with binding
 * b = lane_binding[root[l]]:
 *   first_sat[l - first] = the smallest model m with bit m of allowed[b] set (NULL
 *     allowed: every model) under which EVERY path entry holds; MG_BV_NO_MODEL when
 *     there is none; MG_PATH_UNKNOWN when the lane is unknown (below);
 *   sat_bits (may be NULL) has mg_eval_bits' layout, one bit per satisfying allowed
 *     model; all zero for an unknown lane.
 * A lane with path_len == 0 is satisfied by every allowed model.  `allowed`
 * carries what does not depend on the path (the lineage's initial constraints,
 * the keccak conjunct): the sat_bits rows mg_eval_bits gave for them, unchanged.
 * An entry (cond_tag, side) with condition node c = cond_tag - 1 holds when
 * (value(c) != 0) == (side == 1): fork_conditions' rules.  models == NULL uses the
 * pool the last mg_eval_upload (or mg_eval*, or mg_explore_check with models) left
 * resident; otherwise the models are uploaded as mg_eval uploads them, and the
 * programs of an earlier mg_eval_upload are dropped (mg_eval_run then gives
 * MG_ESTATE: they may name variables the new pool does not have).
 *
 * The value of a node under model m is an integer masked to the node's width
 * (x >> 8, 1..256), the value of the term the host's decoder builds for the node
 * as kernel 2 computes it (z3's x / 0, x mod 0, signed division and shifts >= the
 * width are kernel 2's).  An operand ref with MG_SYM_CONST is the lane's constant,
 * otherwise a node's value; a node only refers to nodes below itself.
 *   MG_SYM_CDSIZE        values[var_cdsize][m]
 *   MG_SYM_ENV, w < MG_ENV_WORDS   values[var_env[w]][m]
 *   calldata byte at the 256-bit index i: i < size (signed, as state/calldata.py's
 *     bound check) ? table tab_calldata at i : 0
 *   MG_SYM_CDLOAD(y)     the big-endian bytes at value(y) + k mod 2^256, k = 0..31
 *   MG_SYM_CDBYTE        the byte at w;  MG_SYM_CDBYTEX: at value(y) + w mod 2^256
 *   MG_SYM_BIN           ADD MUL SUB; DIV SDIV MOD SMOD = bvudiv bvsdiv bvurem
 *     bvsrem; LT GT (unsigned) SLT SGT EQ (0 / 1); AND OR XOR; BYTE with a constant
 *     index y below 32; SHL SHR SAR with the amount in y
 *   MG_SYM_UN            ISZERO: value(y) == 0; NOT: the complement at the width
 *   MG_SYM_EXTRACT       bits w >> 16 .. w & 0xffff of node y (the node's width is
 *     their count); MG_SYM_CONCAT: y high, z low, widths w & 0xffff and w >> 16
 *     (the node's width is their sum, at most 256)
 *   MG_SYM_SLOAD(y, z)   the store chain walked from entry z - 1 down to 0: the
 *     first entry whose key's value equals value(y) gives its value's value (a tag
 *     of 0: the limbs of the storage row, else node tag - 1); no match: table
 *     tab_storage at value(y) on an MG_LANE_SYMSTORE lane, else 0
 * A lane is MG_PATH_UNKNOWN -- a normal answer, one per lane whatever the model --
 * when the cone of its path's condition nodes (what operand refs and, for SLOAD,
 * the store-chain tags reach) holds MG_SYM_KECCAK, MG_SYM_TERM, MG_SYM_MLOADK,
 * MG_SYM_MSTOREK or MG_SYM_BALANCE; an MG_SYM_ENV with w >= MG_ENV_WORDS; a BIN /
 * UN opcode not listed (EXP's Power), a BYTE whose index is no constant below 32,
 * an unknown kind or a width outside what is stated above; a symbol whose binding
 * field is MG_PATH_UNBOUND, a lineage whose lane_binding is MG_PATH_UNBOUND or a
 * root outside the batch; a reference at or past n_nodes / n_consts or not below
 * the referring node, z above the lane's storage_count, a cond_tag of 0, or an
 * arena of more than MG_PATH_MAX_NODES nodes.  Every index the kernel follows is
 * checked against the lane's counts and the planes' capacities before it is used.
 * Nodes outside the cone never matter.
 *
 * Checked on the host (MG_EINVAL, nothing launched, nothing written): an entry of
 * lane_binding that is neither below n_bindings nor MG_PATH_UNBOUND; a binding's
 * variable / table index that is neither below the pool's counts nor
 * MG_PATH_UNBOUND; first + n > n_lanes; NULL first_sat, bindings (with
 * n_bindings > 0) or lane_binding with n > 0; a pool of no models.  n == 0
 * succeeds.  The number of launches and copies does not depend on n.          */
#define MG_PATH_UNKNOWN 0xfffffffeu   /* first_sat[]: the path needs a term the device does not evaluate */
#define MG_PATH_UNBOUND 0xffffffffu   /* a binding field / lane_binding[]: nothing bound */
#define MG_PATH_MAX_NODES 65536u      /* largest arena (n_nodes) mg_explore_check evaluates */
typedef struct mg_path_binding {      /* where one lineage's symbols live in the model batch */
    uint32_t var_cdsize;              /* {id}_calldatasize: index into models->values */
    uint32_t tab_calldata;            /* {id}_calldata: table index (Array 256 -> 8) */
    uint32_t var_env[MG_ENV_WORDS];   /* by MG_ENV_ADDRESS .. MG_ENV_GASPRICE */
    uint32_t tab_storage;             /* Storage{addr} (Array 256 -> 256) for MG_LANE_SYMSTORE lanes */
} mg_path_binding;
struct mg_model_batch;
int         mg_explore_check(mg_ctx *ctx, const struct mg_model_batch *models,
                             const mg_path_binding *bindings, uint32_t n_bindings,
                             const uint32_t *lane_binding /* [n_lanes], indexed by root[lane] */,
                             const uint64_t *allowed /* [n_bindings][ceil(n_models/64)] or NULL */,
                             uint32_t first, uint32_t n,
                             uint32_t *first_sat /* [n] */, uint64_t *sat_bits /* [n][ceil(n_models/64)] or NULL */,
                             float *kernel_ms);

/* mg_explore_check with the models' uninterpreted functions bound: the tables of
 * keccak256_<bits> and Power, which the pool carries as kernel 2 reads them (keys
 * as smt/lower.py's TableSig.key_chunks makes them: one argument x of at most 512
 * bits is (x mod 2^256, x >> 256), two arguments of at most 256 bits each are
 * (first, second)).  Everything stated for mg_explore_check holds; mg_explore_check
 * is this call with functions == NULL, and NULL is the same as a struct with
 * nothing bound: MG_SYM_KECCAK and EXP's Power in a cone are then MG_PATH_UNKNOWN.
 * The functions are the pool's, not a lineage's: one struct per call.
 *
 * Two more rules give values (each table read is part 0, and gives the table's
 * default for that model when no entry matches):
 *   MG_SYM_KECCAK(y, w)  node width 256; with x the input's value as a w-bit
 *     integer, the table bound for width w at (x mod 2^256, x >> 256).  The input y
 *     is a constant (w <= 256, masked to w), a node of width exactly w that the
 *     rules above evaluate, or a tree of MG_SYM_CONCAT nodes: y high, z low, widths
 *     w & 0xffff and w >> 16, each at least 1, their sum the node's width, which
 *     inside such a tree may be 257..512; each operand is again a constant of at
 *     most 256 bits, a node of exactly the stated width, or a CONCAT.  Any tree
 *     shape is taken (sym_mem_ref's left-leaning chains, the host encoder's own), up
 *     to MG_PATH_KECCAK_LEAVES leaves.
 *   MG_SYM_BIN, w == 0x0a  node width 256: table tab_power at (value(y), value(z)),
 *     y the base (first pop) and z the exponent, as symbolic.binary builds
 *     Power(base, exponent).
 * A lane is also MG_PATH_UNKNOWN when its cone holds an MG_SYM_KECCAK whose w is 0,
 * above 512 or a width no table is bound for, whose node width is not 256, or whose
 * input has more than MG_PATH_KECCAK_LEAVES leaves, a reference not below its
 * referrer or past n_consts, or a node whose width is not the one its referrer
 * states (w for y; a CONCAT's w for its operands); an input that is an
 * MG_SYM_MLOADK (or holds any node the rules do not evaluate); Power with
 * tab_power unbound.  A CONCAT wider than 256 bits has no value of its own: reached
 * any other way than through a KECCAK input (a path condition, a BIN operand, an
 * EXTRACT source, a chain tag) it makes the lane unknown, as in mg_explore_check.
 *
 * What stays with the caller, through `allowed`: the keccak conjunct (whichever
 * registrations it covers), exponent_function_manager's side conditions and the
 * result == Power(b, e) constraints of concrete EXP records.  The device evaluates
 * the path's own entries and nothing else.
 *
 * Checked on the host with the rest (MG_EINVAL, nothing launched, nothing
 * written): n_keccak above MG_PATH_KECCAK_WIDTHS; a bound width of 0 or above 512;
 * a repeated width; tab_power or a keccak_tab entry that is neither below the
 * pool's table count nor MG_PATH_UNBOUND.  Entries at and above n_keccak are not
 * read.  The struct travels with the call's other arrays: the number of launches
 * and copies is mg_explore_check's.                                              */
#define MG_PATH_KECCAK_WIDTHS 8u      /* keccak256_<bits> tables one call binds */
#define MG_PATH_KECCAK_LEAVES 64u     /* most leaves of a KECCAK input tree (a 512-bit input of whole bytes) */
typedef struct mg_path_functions {    /* where the uninterpreted functions live in the model batch */
    uint32_t tab_power;               /* Power (256, 256) -> 256: table index, or MG_PATH_UNBOUND */
    uint32_t n_keccak;                /* <= MG_PATH_KECCAK_WIDTHS */
    uint32_t keccak_bits[MG_PATH_KECCAK_WIDTHS];   /* input widths, 1..512, distinct */
    uint32_t keccak_tab[MG_PATH_KECCAK_WIDTHS];    /* table of keccak256_<bits>, or MG_PATH_UNBOUND */
} mg_path_functions;
int         mg_explore_check_fn(mg_ctx *ctx, const struct mg_model_batch *models,
                                const mg_path_binding *bindings, uint32_t n_bindings,
                                const uint32_t *lane_binding /* [n_lanes], indexed by root[lane] */,
                                const uint64_t *allowed /* [n_bindings][ceil(n_models/64)] or NULL */,
                                const mg_path_functions *functions /* or NULL: nothing bound */,
                                uint32_t first, uint32_t n,
                                uint32_t *first_sat /* [n] */, uint64_t *sat_bits /* [n][ceil(n_models/64)] or NULL */,
                                float *kernel_ms);

/* Replaces the LaserEVM.exec() drain for device-eligible lanes (svm.py:293-337
 * + execute_state svm.py:369-491 + Instruction.evaluate instructions.py:235-267):
 * steps every RUNNING lane until it halts, escapes, reaches an opcode whose bit
 * is set in hook_mask (bit b of hook_mask[b>>6]), or has executed max_steps
 * instructions in this call.  max_depth: states with depth >= max_depth are
 * dropped (0 = unlimited).                                                   */
int         mg_step(mg_ctx *ctx, const uint64_t hook_mask[4], uint32_t max_steps,
                    uint32_t max_depth, mg_step_stats *stats);
/* BoundedLoopsStrategy (bounded_loops.py:84-145) on the device: with bound > 0
 * (and a batch allocated with trace_cap > 0) every instruction a lane is popped
 * at is appended to its trace, and at a JUMPDEST a lane whose loop count
 * (get_loop_count) exceeds the bound stops with MG_LOOP_BOUND; creation lanes
 * only when the count also reaches 128.  0 turns it off.                      */
int         mg_set_loop_bound(mg_ctx *ctx, uint32_t bound);
/* Same, with a step horizon: a lane also pauses (stays MG_RUNNING) once its
 * cumulative `steps` reaches `horizon` (0 = none).  The host layer uses it to
 * deliver hook and halt events in the reference's BFS round order
 * (mythril_amd/laser/svm.py).                                                */
int         mg_step_until(mg_ctx *ctx, const uint64_t hook_mask[4], uint32_t max_steps,
                          uint32_t max_depth, uint32_t horizon, mg_step_stats *stats);
/* n_batches whole batches enqueued back to back with one host wait: for each,
 * mg_lanes_reset then one stepping launch, statistics into stats[b] (kernel_ms
 * = the sequence's device time / n_batches, launch gaps included; with
 * MG_BATCH_EVENTS=1 each launch is bracketed instead).  Same preconditions as
 * mg_lanes_reset.                                                           */
int         mg_run_batches(mg_ctx *ctx, const uint64_t hook_mask[4], uint32_t max_steps,
                           uint32_t max_depth, uint32_t n_batches, mg_step_stats *stats);
/* Profiling variant (the InstructionProfiler plugin's per-opcode counts,
 * instruction_profiler.py:41-115, as native counters): op_counts[256] =
 * instructions executed per opcode byte; extra[4] = {SHA3 input bytes,
 * CALLDATACOPY/CODECOPY bytes, storage entries scanned, Keccak blocks}.     */
int         mg_step_profile(mg_ctx *ctx, const uint64_t hook_mask[4], uint32_t max_steps,
                            uint32_t max_depth, uint64_t *op_counts, uint64_t *extra);
/* Same, asynchronous: enqueue only (no stats, no host sync).                */
int         mg_step_async(mg_ctx *ctx, const uint64_t hook_mask[4], uint32_t max_steps,
                          uint32_t max_depth);
int         mg_sync(mg_ctx *ctx);

/* Coverage plugin state (coverage_plugin.py:68-85): one byte per instruction
 * index, 1 = executed by some lane since the last mg_coverage_clear.         */
int         mg_coverage(mg_ctx *ctx, uint32_t code_id, uint8_t *bytes, uint32_t n);
int         mg_coverage_clear(mg_ctx *ctx);

/* Number of Keccak-256 evaluations (SHA3 with concrete input) and EXP
 * evaluations per lane since upload/reset: the host re-registers them with
 * keccak_function_manager / exponent_function_manager when it materialises a
 * lane as a GlobalState (keccak_function_manager.py:95-114).                 */
int         mg_event_counts(mg_ctx *ctx, uint32_t *sha3_count, uint32_t *exp_count,
                            uint32_t first, uint32_t n);

/* -------------------------------------------------- constraint prefilter */
/* A batch of constraint sets, each compiled by the host into a register
 * program over 256-bit values (mythril_amd/smt/flatten.py).  Replaces the
 * model loop of ModelCache.check_quick_sat (support_utils.py:60-68).
 * Instruction: op | width << 8 | store << 17 | slot << 18, then three operand
 * refs (kind << 30 | index; kind 0 = the accumulator, 1 slot, 2 variable,
 * 3 constant) or immediates.  Since ABI 8 only operand A may be the
 * accumulator (the flattener swaps / reverses / spills): a program with the
 * accumulator in operand B or C is refused with MG_EINVAL, and so is one
 * with any of bits 22..31 of the first word set (the library's own fused
 * forms use them: it rewrites common instruction pairs and chains into
 * superinstructions at upload, bit-identical results; MG_BV_FUSE=0 disables).
 *
 * The opcodes, X(C name, name in the host's expression layer).  The result lands
 * in the accumulator; A, B, C = the operands of words 1..3.                   */
#define MG_BV_OP_LIST(X) \
    X(COPY, "copy")               /* acc = A */ \
    X(ADD, "bvadd") X(SUB, "bvsub") X(MUL, "bvmul") X(UDIV, "bvudiv") X(UREM, "bvurem") \
    X(SDIV, "bvsdiv") X(SREM, "bvsrem") X(SMOD, "bvsmod") \
    X(AND, "bvand") X(OR, "bvor") X(XOR, "bvxor") X(NOT, "bvnot") X(NEG, "bvneg") \
    X(SHL, "bvshl") X(LSHR, "bvlshr") X(ASHR, "bvashr") \
    X(EQ, "eq") X(ULT, "bvult") X(ULE, "bvule") X(UGT, "bvugt") X(UGE, "bvuge") \
    X(SLT, "bvslt") X(SLE, "bvsle") X(SGT, "bvsgt") X(SGE, "bvsge")   /* w3 = operand width */ \
    X(BAND, "and") X(BOR, "or") X(BXOR, "xor") X(BNOT, "not") X(BIMPLIES, "implies") \
    X(ITE, "ite")                 /* A cond, B then, C else */ \
    X(EXTRACT, "extract")         /* A, w2 = lo */ \
    X(CONCAT, "concat")           /* A high, B low, w3 = width of B */ \
    X(ZEXT, "zero_extend")        /* A (value already masked) */ \
    X(SEXT, "sign_extend")        /* A, w2 = source width */ \
    X(ADD_NOOVF_U, "bvadd_noovfl_u")   /* bvadd_noovfl unsigned; w3 = operand width */ \
    X(MUL_NOOVF_U, "bvumul_noovfl")    /* bvumul_noovfl;        w3 = operand width */ \
    X(SUB_NOUDF_U, "bvsub_noudfl_u")   /* BVSubNoUnderflow unsigned: b <= a */ \
    X(NE, "distinct")             /* w3 = operand width */ \
    X(TAB, "tab")                 /* A = key k0, B = key k1, w3 = table | part << MG_BV_TAB_PART_SHIFT | \
                                     lo << MG_BV_TAB_LO_SHIFT: bits [256 part + lo, +width) of the model's \
                                     array / function interpretation at (k0, k1), else its default */ \
    X(UMIN, "bvumin") X(UMAX, "bvumax")   /* ite(cmp(A, B), A, B) folded by the compiler */ \
    X(SMIN, "bvsmin") X(SMAX, "bvsmax")   /* signed at `width` */ \
    X(RSUB, "bvrsub")             /* B - A           (operand-swapped forms: the accumulator is only */ \
    X(RCONCAT, "rconcat")         /* A low, B high,   ever operand A; w3 = width of A) */
#define MG_BV_ENUM_(name, host) MG_BV_##name,
enum { MG_BV_OP_LIST(MG_BV_ENUM_) MG_BV_NUM_OPS };   /* MG_BV_COPY = 0, ... */
#undef MG_BV_ENUM_
#define MG_BV_REF_ACC   0u   /* operand reference kinds */
#define MG_BV_REF_SLOT  1u
#define MG_BV_REF_VAR   2u
#define MG_BV_REF_CONST 3u
#define MG_BV_MAX_SLOTS  16u    /* the 4-bit slot field                          */
#define MG_BV_TILE_INSNS 2048u  /* longest program, in instructions              */
#define MG_BV_TAB_INDEX_MASK 0xfffffu   /* MG_BV_TAB's immediate: table index,   */
#define MG_BV_TAB_PART_SHIFT 20         /* 256-bit half of the 512-bit value,    */
#define MG_BV_TAB_LO_SHIFT   21         /* low bit within it                     */
typedef struct mg_dag_batch {
    uint32_t n_dags;
    uint32_t n_slots;       /* register slots a program may use (<= 16)       */
    const uint32_t *prog_off;   /* [n_dags+1] offsets into `insns`            */
    const uint32_t *insns;      /* [total][4] encoded instructions            */
    const uint32_t *consts;     /* [n_consts][8] 256-bit constants            */
    uint32_t n_consts;
} mg_dag_batch;

/* Candidate models, most-recently-used first (LRU order of
 * support_utils.py:62-63).  Variables absent from a model take 0
 * (z3 model_completion).  The values table (n_vars x
 * n_models x 32 bytes) must stay under 4 GiB: the kernel addresses it with
 * 32-bit offsets, and a larger one is refused with MG_EINVAL.
 *
 * Tables are the models' interpretations of symbolic arrays (storage,
 * calldata, balances: array.py) and uninterpreted functions (keccak256_N and
 * its inverse, Power: function.py), looked up by the program op MG_BV_TAB.  For
 * table t and model m, entries [tab_start[t][m], + tab_count[t][m]) of
 * tab_entries hold (key k0: 8 limbs, key k1: 8 limbs, value: 16 limbs, i.e. up
 * to 512 bits); a key not listed takes tab_default[t][m] (array default /
 * function else value).                                                     */
typedef struct mg_model_batch {
    uint32_t n_models;
    uint32_t n_vars;
    const uint32_t *values;     /* [n_vars][n_models][8]                      */
    uint32_t n_tables;          /* 0: no tables (pointers below ignored)      */
    const uint32_t *tab_start;  /* [n_tables][n_models]                       */
    const uint32_t *tab_count;  /* [n_tables][n_models]                       */
    const uint32_t *tab_entries;/* [n_entries][32]                            */
    uint32_t n_entries;
    const uint32_t *tab_default;/* [n_tables][n_models][16]                   */
} mg_model_batch;

/* first_sat_model[d] = smallest model index m (MRU order) whose evaluation of
 * DAG d is true, MG_BV_NO_MODEL if none; sat_count[d] = number of satisfying
 * models (may be NULL).                                                      */
#define MG_BV_NO_MODEL 0xffffffffu
int         mg_eval(mg_ctx *ctx, const mg_dag_batch *dags, const mg_model_batch *models,
                    uint32_t *first_sat_model, uint32_t *sat_count, float *kernel_ms);

/* Same, plus the full satisfaction bitmap: bit m of sat_bits[d][m / 64] is set
 * when model m satisfies DAG d (sat_bits: [n_dags][ceil(n_models / 64)]).  With
 * it the host replays a sequence of check_quick_sat calls exactly, including
 * the LRU moves of returned models between calls (support_utils.py:60-68).    */
int         mg_eval_bits(mg_ctx *ctx, const mg_dag_batch *dags, const mg_model_batch *models,
                         uint32_t *first_sat, uint32_t *sat_count, uint64_t *sat_bits,
                         float *kernel_ms);

/* Device-resident variant used by the benchmark: upload once, evaluate many
 * times without host traffic. */
int         mg_eval_upload(mg_ctx *ctx, const mg_dag_batch *dags, const mg_model_batch *models);
int         mg_eval_run(mg_ctx *ctx, uint32_t dag_first, uint32_t dag_count, float *kernel_ms);
int         mg_eval_download(mg_ctx *ctx, uint32_t *first_sat_model, uint32_t *sat_count,
                             uint32_t dag_first, uint32_t dag_count);

/* Term values.  Replaces model.eval(expr, model_completion=True) of a term
 * under a model (analysis/solver.py:88-93, 191-194), for every (program, model)
 * pair in one launch: values[d][m] = the final accumulator of program d under
 * model m, 8 little-endian 32-bit limbs (a Boolean program leaves 0 or 1).
 * The values (n_dags x n_models x 32 bytes) must stay under 4 GiB (32-bit
 * offsets in the kernels), else MG_EINVAL.                                   */
int         mg_eval_terms(mg_ctx *ctx, const mg_dag_batch *dags, const mg_model_batch *models,
                          uint32_t *values /* [n_dags][n_models][8] */, float *kernel_ms);

/* Lexicographic minimum over the candidate models.  Replaces Optimize.minimize
 * per term + check (support/model.py:56-82; get_transaction_sequence's calldata
 * sizes and call values in priority order, analysis/solver.py:219-259) over the
 * pool: per query, a model is a candidate when every constraint program listed
 * for it evaluates to true (no program listed: every model), and the winner is
 * the candidate with the smallest objective tuple -- each objective an unsigned
 * 256-bit number, the tuple compared in list order, ties to the smallest model
 * index.  Constraint and objective programs are DAGs of the one `dags` batch.
 * best_model[q] = the winner (MG_BV_NO_MODEL: no candidate, then every limb of its
 * values is all-ones), best_values[obj_off[q] + j] = its j-th objective,
 * cand_count[q] = the number of candidates.  Offsets start at 0 and do not
 * decrease, indices are below n_dags, a query lists at most MG_MIN_OBJ
 * objectives: anything else is MG_EINVAL before any launch.                  */
#define MG_MIN_OBJ 8u
typedef struct mg_min_batch {
    uint32_t n_queries, _pad;
    const uint32_t *cons_off;  /* [n_queries+1] into cons_dag                          */
    const uint32_t *cons_dag;  /* DAG indices that must all evaluate to true            */
    const uint32_t *obj_off;   /* [n_queries+1] into obj_dag; <= MG_MIN_OBJ per query   */
    const uint32_t *obj_dag;   /* DAG indices of the minimised terms, most significant first */
} mg_min_batch;
int         mg_eval_min(mg_ctx *ctx, const mg_dag_batch *dags, const mg_model_batch *models,
                        const mg_min_batch *queries, uint32_t *best_model,
                        uint32_t *best_values /* [obj_off[n_queries]][8] */, uint32_t *cand_count,
                        float *kernel_ms);

/* ------------------------------------------------------ conjunct compiler */
/* Kernel 2's register programs compiled on the host from lowered constraint
 * DAGs (mythril_amd/smt/flatten.py's passes in native code; replaces the
 * Python compile of every quick-sat query's conjuncts, support/model.py:48-56
 * -> get_model's And(constraints)).  Nodes are registered once each into a
 * growing table (ids only grow), programs are compiled per conjunct root.
 * Host only: no device, no context needed.                                  */
typedef struct mg_cc mg_cc;
int         mg_cc_open(mg_cc **out);
void        mg_cc_close(mg_cc *cc);
const char *mg_cc_error(mg_cc *cc);
/* rows: n x {op, width, first_arg, n_args, imm}; op = a kernel-2 opcode
 * (MG_BV_*), or MG_CC_VAR (imm = its model-pool index) / MG_CC_CONST (imm =
 * its constant-pool index).  args[first_arg ..]: node ids, or 0x80000000 | k
 * for row k of this call.  ids[i] <- row i's id (an equal existing node's id
 * when there is one).  imm: the low bit of an extract; a table lookup's
 * MG_BV_TAB immediate.                                                      */
#define MG_CC_VAR   0x1000u
#define MG_CC_CONST 0x1001u
int         mg_cc_add(mg_cc *cc, const uint32_t *rows, uint32_t n, const uint32_t *args, uint32_t n_args,
                      uint32_t *ids);
/* The program of the conjunct rooted at node `root`: n_insns x 4 u32 into
 * insns (cap instructions); *max_slots is raised to the slots it uses.
 * MG_EUNSUPPORTED: more than MG_BV_MAX_SLOTS live values, more than
 * MG_BV_TILE_INSNS instructions or a value wider than 256 bits (the set stays
 * with the SMT backend).                                                    */
int         mg_cc_compile(mg_cc *cc, uint32_t root, uint32_t *insns, uint32_t cap, uint32_t *n_insns,
                          uint32_t *max_slots);

#ifdef __cplusplus
}
#endif
#endif /* MYTHGPU_H */
