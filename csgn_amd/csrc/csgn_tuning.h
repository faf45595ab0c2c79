// csgn_tuning.h -- the library's tuning knobs (kernel choice and sweep parameters).
//
// Every knob is one int PER HOST THREAD (thread_local): setting it changes the calling thread's later
// dispatches and nobody else's.  Its start value in every thread is the built-in default, or the
// value of the environment variable CSGN_<KEY IN CAPITALS> sampled ONCE when libcsgn_hip.so is
// loaded; after that only csgn_set_tuning()/csgn_reset_tuning() (include/csgn_hip.h) change it.
// No compute entry point reaches getenv.  Knobs select among kernels that compute the same
// words: results never depend on them.  The GPU tests drive the forms through them: tests/test_gpu_parity.py (the
// multiply, encrypt, decrypt, permutation, compaction and ragged forms), each operation's own tests/test_*_gpu.py and
// class-level tests/test_*_cpp.py (its form knob), tests/test_launch_split_gpu.py (launch_blocks),
// tests/test_block_order_gpu.py (stream_xcd), tests/test_ragged_order_gpu.py (the ragged block orders and slices) and
// tests/test_knob_forms_gpu.py (mul_bs, mul_xcd = 2, the compaction's grid, shared_gpu).  tests/test_tuning_ledger.py
// names the file for every knob and fails for a knob that none sets; zero_memset is the one exemption.
#pragma once

namespace csgn {

enum TuneKey {
    TUNE_MUL_M,          // tiled multiply: column units per lane, 0 = auto
    TUNE_MUL_TI,         // tiled multiply: left terms per LDS tile
    TUNE_MUL_NT,         // tiled multiply: 1 = non-temporal stores
    TUNE_MUL_FLAT,       // 0 = choose per shape; k > 0 = flat kernel, k units per lane; -1 = tiled kernel
    TUNE_MUL_BS,         // tiled multiply: block size override (0 = auto)
    TUNE_MUL_XCD,        // XCD-contiguous block order: 0 off, 1 flat kernel, 2 both kernels
    TUNE_MUL_TOUCH,      // operand touch pass: -1 = per shape, 0..3 = bit 0 left, bit 1 right operand
    TUNE_MUL_PF_KB,      // flat multiply without touch: left-term prefetch distance in KiB, -1 = auto
    TUNE_STREAM_XCD,     // 1x1 multiply / uniform add block order: -1 = by size, 0 / 1 forced
    TUNE_RAGGED_C,       // flat ragged kernels: 4 KiB chunks per workgroup, 0 = auto
    TUNE_RAGGED_FLAT,    // 1 = never use the tiled kernel for ragged batches
    TUNE_RAGGED_PF,      // ragged multiply: operand prefetch distance in pairs, 0 = off
    TUNE_RAGGED_TOUCH,   // ragged multiply: 1 = touch pass per 1 GiB output slice
    TUNE_RAGGED_M,       // flat ragged multiply: 4 KiB chunks per turn that share one speculative pair lookup and whose operand loads travel together: 1, 2 or 4
    TUNE_PERM_BALLOT,    // 1 = ballot bit-gather permutation kernel instead of the bit-plane kernel
    TUNE_PERM_NARROW,    // 1 = 8-byte staging accesses in the bit-plane kernel
    TUNE_PERM_WAVES,     // bit-plane kernel: waves per 64-term group; 0 = auto
    TUNE_PERM_PERSIST,   // bit-plane kernel: 1 = persistent workgroups striding over the groups, 0 = one group per workgroup, k > 1 = k groups per CU resident
    TUNE_DEC_LOOP,       // 1 = looping 256-term decrypt pass 1 instead of the segment form
    TUNE_ENC_LDS,        // 1 = LDS-staged encrypt kernel instead of the segment form
    TUNE_ENC_WAVE,       // device-RNG encrypt: 1 = wave-local kernel (default), 0 = segment kernel
    TUNE_ENC_COMPACT,    // keyed encrypt: compact LDS tables: -1 = auto (groups of 3+ passes), 0 / 1 forced
    TUNE_SHARED_GPU,     // 1 = other work streams through this GPU's HBM beside the caller: all-pairs multiplies take the LDS-tiled kernel instead of the operand-touch + flat pair, which depends on the memory-side cache (include/csgn_hip.h, "Sharing the GPU")
    TUNE_COMPACT_TAG_BITS, // compaction: hash-tag bits the tables keep, 0 = all (a test narrows them to force the collision path)
    TUNE_COMPACT_NT,     // compaction: 1 = non-temporal stores of the surviving terms
    TUNE_COMPACT_GRID,   // compaction: workgroups of the main kernel, 0 = 512 (two per CU)
    TUNE_RAGGED_CLASSES, // planned ragged multiply: 1 = the plan lists small pairs by size class and the multiply gives every class its own tiled launch (measured slower than the CSR kernel: off by default)
    TUNE_RAGGED_COOP,    // ragged multiply of small pairs: 1 = the wave-cooperative kernel (a wave walks its pairs together: no per-lane search or division), 0 = the CSR kernel, -1 = auto (the default: ranges that average 16 product terms a pair and more)
    TUNE_RAGGED_COOP_SPAN, // ... 64-unit blocks of output per wave (0 = 64)
    TUNE_RAGGED_COOP_K,  // ... blocks per group of the software pipeline: 2 or 4 (0 = 4)
    TUNE_RAGGED_COOP_TOUCH, // ... a wave touches the operands of an offset window.s pairs when it loads the window (one dword per 128-byte line): KiB a side at most, 0 = off
    TUNE_RAGGED_SLICE_MB, // ragged multiply: output slice size in MiB, each slice behind a touch of its operands (0 = by the operand share: 1 GiB, 512 MiB or unsliced)
    TUNE_RAGGED_COOP_PIPE, // ... 1 = software-pipelined form (loads of the next group in front of the stores of this one; hand-counted waits), 0 = loads, wait, stores (the default: level with the pipelined form since the operand touch)
    TUNE_RAGGED_XCD_GROUP, // CSR multiply / add: logical blocks per XCD turn (xcd_grouped_block); 0 = one contiguous eighth of the launch per XCD
    TUNE_RAGGED_COOP_XCD_GROUP, // wave-cooperative multiply: workgroups per XCD turn (xcd_grouped_block); 0 = contiguous eighths
    TUNE_COMPACT_STAGGER_US, // compaction: microseconds by which every second workgroup of the main kernel starts late (phases of the two workgroups of a CU interleave), 0 = together
    TUNE_ZERO_MEMSET,    // dev: 1 = zero fills on capturable paths are hipMemsetAsync (memset NODES in a circuit's graph) instead of the k_zero_words kernel (csgn_device.h, zero_words; tools/graph_memset_probe.hip)
    TUNE_GATE_FUSED,     // uniform gates (csgn_gates.hip): -1 = per shape, 0 = pitched form (the tuned launchers into the output's slices), 1 = fused kernel
    TUNE_UINT_FUSED,     // integer steps (csgn_uint.hip): -1 = per shape, 0 = pitched form where the step has one, 1 = fused kernel
    TUNE_UINT_PLAIN_FUSED, // comparisons with a public constant (csgn_uint_plain.hip): -1 = per shape, 0 = composed form (the tuned launchers level by level), 1 = fused kernel
    TUNE_UINT_LUT_FUSED, // public lookup tables (csgn_uint_lut.hip): -1 = per shape, 0 = composed form (the tuned launchers monomial by monomial), 1 = fused kernel
    TUNE_UINT_READ_FUSED, // encrypted tables read at encrypted indices (csgn_uint_read.hip): -1 = per shape, 0 = composed form (the tuned launchers row by row), 1 = fused kernel
    TUNE_UINT_ADDK_FUSED, // integer + public constant (csgn_uint_addk.hip): -1 = per shape, 0 = composed form (the tuned launchers plane by plane), 1 = fused kernel
    TUNE_UINT_ADD_WHERE_FORM, // knob "uint_add_where_form": addWhere, subWhere, incrementWhere and decrementWhere of the classes (certfhe/UInt.h): -1 = per shape, 0 = the loop over the planes through the batch operators, 1 = one csgn_uint_add_where call where it can run; the C call itself is always the kernel
    TUNE_UINT_FIND_FORM, // encrypted tables looked up by encrypted key (csgn_uint_find.hip): -1 = per shape, 0 = composed form (the tuned launchers row by row), 1 = fused kernel
    TUNE_UINT_FIND_RPARTS, // ... row parts of one k_uint_find launch at most, 0 = what a launch's workgroups allow (every shape within memory: one launch); a test sets it low to run the host's split of the rows into several launches
    TUNE_MATMUL_FORM,    // products of encrypted bit matrices (csgn_matmul.hip): -1 = per shape, 0 = composed form (both operands tiled by the gather launcher, one uniform multiply), 1 = fused kernel
    TUNE_MATMUL_EPART,   // ... values of e one k_matmul workgroup takes at most, 0 = by the shape (what the LDS holds, cut further until the workgroups fill the chip); a test sets it to choose where the range of e is split
    TUNE_COUNT_FORM,     // encrypted bits counted into integers (csgn_count.hip): -1 = per shape, 0 = composed form (the factors tiled by the gather launcher, uniform multiplies), 1 = fused kernel
    TUNE_COUNT_CPART,    // ... combination ranks one k_count workgroup takes at most, 0 = by the shape (what its subset table holds, cut further until the workgroups fill the chip), and one k_count_prefix workgroup (csgn_count_prefix.hip) of the ranks of a plane's rows together; a test sets it to place the split of the ranks
    TUNE_WSUM_CPART,     // encrypted integers summed into integers (csgn_wsum.hip): selection ranks one k_wsum workgroup takes at most, 0 = by the shape (what its index table holds, no more than 1024 terms); read when a plan is created; a test sets it to place the split of the ranks
    TUNE_UINT_LT_SELECT_FORM, // selection by an encrypted comparison (csgn_uint_lt_select.hip): -1 = per shape, 0 = composed form (the LT steps and one MUX gate per output through the tuned launchers), 1 = fused kernel
    TUNE_UINT_PICK_FORM, // knob "uint_pick_fused": shifts, rotates and per-element reads by an encrypted amount (csgn_uint_pick.hip): -1 = per shape, 0 = composed form (the tuned launchers row by row), 1 = fused kernel
    TUNE_UINT_PICK_STAGE, // ... the fused kernel copies a workgroup's value units into LDS where they fit: -1 = per shape, 0 = plain global loads, 1 = staged
    TUNE_UINT_WRITE_FORM, // knob "uint_write_fused": encrypted arrays written at encrypted indices (csgn_uint_write.hip): -1 = per shape, 0 = composed form (the tuned launchers row by row), 1 = fused kernel
    TUNE_UINT_PICK_ROWS_FORM, // knob "uint_pick_rows_form": arrays whose rows differ in size read at encrypted indices, the read after csgn_uint_write (csgn_uint_pick_rows.hip): -1 = per shape, 0 = composed form (the tuned launchers row by row), 1 = fused kernel
    TUNE_UINT_DECRYPT_FORM, // knob "uint_decrypt_form": UIntBatch::decrypt and decryptPacked of the classes (certfhe/UInt.h): -1 = per shape, 0 = one CiphertextBatch::decrypt per plane, 1 = one csgn_uint_decrypt call; the C call itself is always the kernel
    TUNE_UINT_DECRYPT_CHUNK, // knob "uint_decrypt_chunk": csgn_uint_decrypt (csgn_uint_decrypt.hip): the most terms of one element of a uniform plane a wave takes before the element is cut into chunks that meet in the value word by atomics, 0 = by shape (1024), never more than 4096; a test sets it low to place the cut
    TUNE_UINT_BITWISE_FORM, // knob "uint_bitwise_form": a & b, a | b, a ^ b, ~a, select and keepWhere of encrypted integers (csgn_uint_bitwise.hip): -1 = per shape, 0 = plane by plane (csgn_gate_uniform's, csgn_mul_uniform's and csgn_add_uniform's launchers), 1 = the one kernel for every plane
    TUNE_UINT_ARITH_FORM, // knob "uint_arith_form": a + b, a - b, a == b, a != b of encrypted integers (csgn_uint_arith.hip): -1 = per shape, 0 = the per-bit chain (csgn_uint_step's and csgn_gate_uniform's launchers plane by plane), 1 = the one launch
    TUNE_LAUNCH_BLOCKS,  // 256-thread workgroups one launch takes at most where the host splits a call into launches (launch_blocks, csgn_device.h), 0 = the HIP limit; a test sets it low to run the host's splits
    TUNE_COUNT
};

int tune(TuneKey k);                      // the calling thread's value
bool tune_choose(TuneKey k, bool by_shape); // a "-1 = by shape, 0 / 1 forced" knob: forced 0 / 1 wins, else by_shape
const char *tune_name(int k);             // "mul_m", ... (nullptr past the end)
bool tune_set(const char *name, int value);
bool tune_get(const char *name, int *value);
void tune_reset();                        // defaults, then the environment snapshot taken at load

} // namespace csgn
