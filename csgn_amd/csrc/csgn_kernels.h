// csgn_kernels.h -- launchers for the gfx950 kernels (internal; the public surface is
// include/csgn_hip.h).
#pragma once

#include "csgn_common.h"

#include <vector>

struct csgn_small_op;   // include/csgn_hip.h

namespace csgn {

// Tunables of the tiled all-pairs kernel; defaults chosen by measurement on MI355X
// ("all-pairs multiply").  Overridable through the environment for sweeps:
// CSGN_MUL_M (column units per lane), CSGN_MUL_TI (left terms per tile),
// CSGN_MUL_NT (1 = non-temporal stores).
struct MulTuning {
    int m;      // CSGN_MUL_M: column units per lane, 0 = auto
    int ti;
    int nt;
    int flat;   // CSGN_MUL_FLAT: 0 = choose per shape (mul_plan); k > 0 = flat kernel, k units per lane; -1 = LDS-tiled kernel
    int bs;     // CSGN_MUL_BS: override the tiled kernel's block size (0 = auto)
    int xcd;    // CSGN_MUL_XCD: XCD-contiguous block order: 0 off, 1 flat kernel only (default), 2 both kernels
};
MulTuning mul_tuning();
// name of the kernel(s) a mul_uniform call of `pairs` pairs of this shape dispatches to
// (16-byte aligned buffers assumed)
const char *mul_uniform_kernel_name(u64 n_bits, u64 pairs, u64 t1, u64 t2);

// out_pitch_words != 0 (circuit placement): element e's product is written at out + e * out_pitch_words instead of
// densely, e.g. into its slice of the sum that consumes it; out_slots is ignored then
hipError_t mul_uniform(u64 n_bits, u64 batch, u64 t1, u64 t2, const u64 *L, const u64 *R, u64 *out,
                       u64 out_slots, hipStream_t s, u64 out_pitch_words = 0);
u64 mul_ragged_plan_scratch_words(u64 batch);
u64 mul_ragged_plan_head_words();       // [plan4][huge-pair count][records][operand terms][offsets checksum]: what the host copies back
// What a plan learned beyond its four numbers; lives in the caller's csgn_mul_plan object.
struct MulPlanNotes {
    const u64 *offL = nullptr, *offR = nullptr, *offOut = nullptr;
    u64 batch = 0, total = 0, max_t1 = 0, max_t2 = 0;
    u64 operand_terms = 0;               // left + right terms of the whole batch
    u64 checksum = 0;                    // of the three offset arrays as planned
    u32 n = 0;                           // huge-pair records kept (sorted by pair)
    u64 rec[32][6];                      // {pair, offL, offR, t1, t2, offOut}
    // size classes of small pairs (csgn_mul.hip, class_of): pairs and product terms per class, and the device
    // list of every class's pairs (class c = lists[cls_base[c] .. cls_base[c + 1])); nullptr: no lists
    u64 cls_pairs[28] = {0}, cls_terms[28] = {0}, cls_base[29] = {0};
    const u32 *lists = nullptr;
};
// d_work: the plan's device block (mul_ragged_plan wrote the class lists there) when it stays alive with the
// notes -- a csgn_mul_plan owns one --, nullptr otherwise
void mul_plan_notes_from_head(MulPlanNotes &notes, const u64 *offL, const u64 *offR, const u64 *offOut, u64 batch,
                              const u64 *h_head, const u64 *d_work);
u32 offsets_checksum_words();          // d_sum of offsets_checksum: this many words, to be added up on the host
hipError_t offsets_checksum(u64 batch, const u64 *offL, const u64 *offR, const u64 *offOut, u64 *d_sum, hipStream_t s);
// gate (csgn_mul_ragged_async only): three device words the last plan kernel fills for the kernels behind it
hipError_t mul_ragged_plan(u64 batch, const u64 *offL, const u64 *offR, u64 *offOut, u64 *d_work,
                           hipStream_t s, u64 *gate = nullptr, u64 capacity_terms = 0, bool can_stream = false);
// notes: what the plan of exactly these offset arrays learned about huge pairs and operand size (nullptr: nothing;
// a circuit's offsets never came from a plan).  operand_terms: left + right terms of the whole batch when the
// caller knows them (a circuit does: its shapes are static), 0 = unknown; sizes the output slices of a large product.
// d_gate: csgn_mul_ragged_async -- {real output terms, ...} left on the DEVICE by the plan kernels; the grid is then
// sized by total_out_terms (the caller's bound) and only the CSR kernel is used.
hipError_t mul_ragged(u64 n_bits, u64 batch, const u64 *L, const u64 *offL, const u64 *R,
                      const u64 *offR, u64 *out, const u64 *offOut, u64 max_t1, u64 max_t2,
                      u64 total_out_terms, hipStream_t s, const MulPlanNotes *notes = nullptr, u64 operand_terms = 0,
                      const u64 *d_gate = nullptr, const u64 *d_huge = nullptr);
// plan + multiply enqueued back to back, nothing read back (csgn_mul_ragged_async); d_plan: mul_ragged_async_plan_words(batch)
u64 mul_ragged_async_plan_words(u64 batch);
hipError_t mul_ragged_async(u64 n_bits, u64 batch, const u64 *L, const u64 *offL, const u64 *R, const u64 *offR,
                            u64 *out, u64 *offOut, u64 capacity_terms, u64 *d_plan, hipStream_t s);
// out_pitch_words != 0 (circuit placement): element e's t1 + t2 terms go to out + e * out_pitch_words; with t1 or t2
// zero (that operand's pointer is then not read) this is the strided copy of one operand into its slice of a sum
hipError_t add_uniform(u64 n_bits, u64 batch, u64 t1, u64 t2, const u64 *L, const u64 *R, u64 *out,
                       hipStream_t s, u64 out_pitch_words = 0);
// device_end: total_terms_out is only an upper bound (sizes the launch); the real end is read from the offsets
// a list of strided copies in one launch (the prologue of a compiled circuit: copies whose sources are circuit inputs)
struct CopyEntry {
    const u64 *src;
    u64 *dst;
    u32 elem_words, src_pitch, dst_pitch, batch;   // words per element, words from element to element, elements
};
u32 copy_list_blocks(const CopyEntry &e);              // workgroups entry e needs
// d_first[e] = first workgroup of entry e (exclusive sums of copy_list_blocks), total_blocks = their sum
hipError_t copy_list(const CopyEntry *d_entries, const u32 *d_first, u32 n_entries, u32 total_blocks, hipStream_t s);
// max_t1 / max_t2: upper bounds on one element's terms (0, 0 = unknown); met with equality = a uniform batch
hipError_t add_ragged(u64 n_bits, u64 batch, const u64 *L, const u64 *offL, const u64 *R,
                      const u64 *offR, u64 *out, u64 *offOut, u64 total_terms_out, hipStream_t s,
                      bool device_end = false, u64 max_t1 = 0, u64 max_t2 = 0);
// A ciphertext of more terms is "long": the ragged pass 2 of decrypt folds it chunk by chunk, and uint_decrypt refuses a
// ragged plane whose bound is above it.
constexpr u64 kLongTerms = 4096;
// max_terms (ragged batches): an upper bound on the terms of one ciphertext, 0 = unknown
hipError_t decrypt(u64 n_bits, u64 batch, u64 terms_uniform, u64 total_terms, const u64 *terms,
                   const u64 *off, const u64 *mask, uint8_t *bits, void *scratch, hipStream_t s, u64 max_terms = 0);
// mod-2 compaction (csgn_compact.hip).  max_terms: an upper bound on the terms of any one ciphertext when
// the caller knows it (0 = unknown); it only decides whether the kernels for ciphertexts larger than a
// workgroup's group are launched at all.
bool compact_supported(u64 n_bits);
size_t compact_scratch_bytes(u64 n_bits, u64 batch, u64 total_terms);
hipError_t compact(u64 n_bits, u64 batch, u64 total_terms, u64 max_terms, const u64 *terms, const u64 *off,
                   u64 *out, u64 *off_out, void *scratch, hipStream_t s);
hipError_t encrypt(u64 n_bits, u64 d, u64 batch, const uint8_t *plain, const u64 *rnd,
                   const u32 *chosen, const uint8_t *last, const u64 *mask, u64 *out, hipStream_t s);
// Keyed (ChaCha) device-RNG encrypt; keystream layout in csgn_encrypt.hip.
hipError_t bump_epoch(u64 *d_epoch, hipStream_t s);      // *d_epoch += 1 (head node of a circuit with encrypt inputs)
void encrypt_keyed_layout(u64 n_bits, u32 *U, u32 *P, u32 *Gc);
hipError_t encrypt_keyed(u64 n_bits, u64 d, u64 batch, u64 first_ct, const uint8_t *plain, const u64 *key_idx,
                         const u64 *mask, const u32 rng_key[8], u64 nonce, u32 rounds,
                         const u64 *d_epoch, u64 *out, hipStream_t s);
// Fused fresh chain: out_c = Enc_A(plain_a[c]) & Enc_B(plain_b[c]) in one kernel, optional Dec of it.
hipError_t encrypt_mul_keyed(u64 n_bits, u64 d, u64 batch, u64 first_ct, const uint8_t *plain_a,
                             const uint8_t *plain_b, const u64 *key_idx, const u64 *mask, const u32 key_a[8],
                             u64 nonce_a, const u32 key_b[8], u64 nonce_b, u32 rounds, const u64 *d_epoch, u64 *out,
                             uint8_t *bits, hipStream_t s);
hipError_t permute(u64 n_bits, u64 batch, u64 terms_in, bool per_term, const u64 *terms,
                   const u32 *perm, u64 *out, hipStream_t s);
// one ciphertext with an explicit bitlen side array (csgn_bitlen.hip)
size_t bitlen_scratch_bytes(u64 len);
hipError_t decrypt_bitlen(u64 n_bits, u64 d, u64 len, const u64 *v, const u64 *bitlen, const u64 *key,
                          uint8_t *bit, void *scratch, hipStream_t s);
hipError_t permute_bitlen(u64 n_bits, u64 len, const u64 *v, const u64 *bitlen, const u32 *perm, u64 *out,
                          void *scratch, hipStream_t s);
hipError_t circuit_zero_words(u64 *p, u64 n, hipStream_t s);   // zero-fill by a kernel (graph-safe, csgn_device.h)
hipError_t synth_fill(u64 seed, u64 n_bits, u64 first_word, u64 n_words, u64 *out, hipStream_t s);
hipError_t digest(const u64 *w, u64 n_words, u64 first_index, u64 *d_digest, hipStream_t s);

// gates over uniform batches and the constant term (csgn_gates.hip); gate = CSGN_GATE_* of include/csgn_hip.h
u64 gate_terms(int gate, u64 ts, u64 ta, u64 tb);                  // 0: bad gate, zero term count or overflow
const char *gate_kernel_name(u64 n_bits, int gate, u64 batch, u64 ts, u64 ta, u64 tb);
// pitch_words: words from one element's constant to the next (0 = dL, a dense batch of 1-term ciphertexts)
hipError_t const_fill(u64 n_bits, u64 batch, const uint8_t *plain, int bit, u64 *out, u64 pitch_words, hipStream_t s);
hipError_t gate_uniform(u64 n_bits, int gate, u64 batch, u64 ts, u64 ta, u64 tb, const u64 *S, const u64 *A,
                        const u64 *B, const uint8_t *plain, u64 *out, hipStream_t s);

// one per-bit step of the bit-sliced integers over uniform batches (csgn_uint.hip); step = CSGN_UINT_* of include/csgn_hip.h
u64 uint_step_terms(int step, int output, u64 tx, u64 ta, u64 tb);   // 0: bad step / output, zero term count or overflow
const char *uint_step_kernel_name(u64 n_bits, int step, u64 batch, u64 tx, u64 ta, u64 tb);
hipError_t uint_step(u64 n_bits, int step, u64 batch, const u64 *X, u64 tx, const u64 *A, u64 ta, const u64 *B, u64 tb,
                     u64 *out0, u64 *out1, hipStream_t s);

// a w-bit comparison of bit-sliced integers against a public constant over uniform planes (csgn_uint_plain.hip);
// cmp = CSGN_UINT_PLAIN_* of include/csgn_hip.h, planes[j] / terms[j]: plane j and its terms per element
u64 uint_plain_terms(int cmp, u64 width, u64 k, const u64 *terms);   // 0: invalid argument or overflow
const char *uint_plain_kernel_name(u64 n_bits, int cmp, u64 batch, u64 width, u64 k, const u64 *terms);
hipError_t uint_plain(u64 n_bits, int cmp, u64 batch, u64 width, u64 k, const u64 *const *planes, const u64 *terms,
                      u64 *out, hipStream_t s);

// a w-bit integer of uniform planes plus a public constant (csgn_uint_addk.hip), include/csgn_hip.h's definition;
// out_terms: width + 1 counts, the last the carry-out's; outs: width planes; carry: nullptr = not computed
bool uint_addk_terms(u64 width, u64 k, const u64 *terms, u64 *out_terms);   // false: invalid argument or overflow
const char *uint_addk_kernel_name(u64 n_bits, u64 batch, u64 width, u64 k, const u64 *terms, bool carry);
hipError_t uint_addk(u64 n_bits, u64 batch, u64 width, u64 k, bool negate_out, const u64 *const *planes, const u64 *terms,
                     u64 *const *outs, u64 *carry, hipStream_t s);

// a public lookup table applied to a w-bit integer of uniform planes (csgn_uint_lut.hip), include/csgn_hip.h's
// definition: output j is the sum, ascending in S, of the monomials M_S of the table's Mobius transform with bit j set.
// A plan compiles one table for one vector of plane term counts; it lives in a csgn_uint_lut object of the caller's.
constexpr u32 kLutMaxIn = 16, kLutMaxOut = 64;
struct LutPlan {
    u32 w = 0, m = 0;                 // in_width, out_width
    u64 t[kLutMaxIn] = {};            // terms per element of plane i
    u64 T[kLutMaxOut] = {};           // terms per element of output j
    u32 mbase[kLutMaxOut + 1] = {};   // output j's monomials: entries [mbase[j], mbase[j + 1]) of the lists
    bool fresh = false;               // every t_i = 1: monomial index = term index
    u32 *d_mono = nullptr;            // the monomial masks, ascending within each output
    u32 *d_moff = nullptr;            // each monomial's first term inside its output (the multi-term decode)
    std::vector<u32> mono;            // host copy of the masks (the composed form)
};
// 0 = CSGN_OK, or a negative csgn_status; the ANF of the table (2^w words)
int uint_lut_anf(u64 w, u64 m, const u64 *table, u64 *anf);
// T_j of every output (m words); CSGN_ERR_INVALID for a bad argument or a count of 2^62 or more
int uint_lut_terms(u64 w, u64 m, const u64 *table, const u64 *t, u64 *T);
// compiles and uploads (synchronous); CSGN_ERR_UNSUPPORTED when an output reaches 2^31 terms
int uint_lut_plan_create(u64 w, u64 m, const u64 *table, const u64 *t, LutPlan &p, hipError_t &herr);
void uint_lut_plan_free(LutPlan &p);
const char *uint_lut_kernel_name(const LutPlan &p, u64 n_bits, u64 batch);
hipError_t uint_lut(const LutPlan &p, u64 n_bits, u64 batch, const u64 *const *planes, u64 *const *out, hipStream_t s);

// gather / tile / broadcast (csgn_gather.hip), include/csgn_hip.h's definition: output element e = source element
// idx[e], or e mod count_in when idx is nullptr.  Counts below 2^32, count_in > 0 when count_out > 0.
constexpr u64 kGatherMaxPlanes = 64;
const char *gather_kernel_name(u64 n_bits, u64 count_out, bool ragged, u64 n_planes);
// synchronous; result[0] = output terms (ragged source), result[1] = bad indices (out_off untouched when nonzero).
// Returns 0, or 1 with herr set.
int gather_plan(u64 count_in, const u64 *src_off, u64 count_out, const u64 *idx, u64 *out_off, u64 result[2],
                hipError_t &herr, hipStream_t s);
// uniform planes, plane j of terms[j] terms per element, every plane in one launch
hipError_t gather_planes(u64 n_bits, u64 n_planes, const u64 *const *src, const u64 *terms, u64 count_in,
                         u64 count_out, const u64 *idx, u64 *const *dst, hipStream_t s);
hipError_t gather_ragged(u64 n_bits, u64 count_in, const u64 *src, const u64 *src_off, u64 count_out, const u64 *idx,
                         u64 *dst, const u64 *out_off, u64 total_terms_out, hipStream_t s);

// an encrypted table read at an encrypted index (csgn_uint_read.hip), include/csgn_hip.h's definition: output j is the
// sum, ascending in r < rows, of EQ(x, r) * d_{r,j}.  index planes: v = 1..16, terms s[k]; table planes: w = 1..64,
// terms t[j].
constexpr u32 kReadMaxIndex = 16, kReadMaxPlanes = 64;
u64 uint_read_terms(u64 v, const u64 *s, u64 rows);   // E; 0: invalid argument or a count of 2^62 or more
const char *uint_read_kernel_name(u64 n_bits, u64 batch, u64 v, const u64 *s, u64 rows, u64 w, const u64 *t);
hipError_t uint_read(u64 n_bits, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 rows, u64 w,
                     const u64 *const *table, const u64 *t, u64 *const *out, hipStream_t stream);

// an encrypted table looked up by encrypted key (csgn_uint_find.hip), include/csgn_hip.h's definition: output j is the
// sum, ascending in r < rows, of EQ(y_r, x) * d_{r,j}, member that of EQ(y_r, x).  key and query planes: v = 1..16,
// terms u[k] / s[k]; value planes: w = 0..64, terms t[j]; member: nullptr = not computed (then w >= 1).
constexpr u32 kFindMaxKey = 16, kFindMaxPlanes = 64;
u64 uint_find_terms(u64 v, const u64 *u, const u64 *s);   // P; 0: invalid argument or a count of 2^62 or more
const char *uint_find_kernel_name(u64 n_bits, u64 batch, u64 v, const u64 *u, const u64 *s, u64 rows, u64 w,
                                  const u64 *t, bool member);
hipError_t uint_find(u64 n_bits, u64 batch, u64 v, const u64 *const *query, const u64 *s, u64 rows,
                     const u64 *const *keys, const u64 *u, u64 w, const u64 *const *values, const u64 *t,
                     u64 *const *out, u64 *member, hipStream_t stream);

// the first row whose encrypted mask bit is set (csgn_uint_first.hip), include/csgn_hip.h's definition: F_r = n_0 * ... *
// n_{r-1} * m_r, output j the sum, ascending in r < g, of F_r * d_{r,j}, any that of F_r, label plane i that of the F_r
// whose public label has bit label_bits[i].  mask: one grouped batch (n_mask == 1) or g batches of `batch` elements, row
// r of s[r] terms; values: w = 0..64 grouped planes, terms t[j]; any, label_out: nullptr / n_labels == 0 = not written.
constexpr u32 kFirstMaxGroup = 64, kFirstMaxPlanes = 64, kFirstMaxLabels = 64;
u64 uint_first_terms(u64 g, const u64 *s, u64 row);    // P_row, Q for row == g; 0: invalid argument or 2^62 or more
u64 uint_first_label_terms(u64 g, const u64 *s, const u64 *labels, u64 bit);   // 0 also where no label has the bit
hipError_t uint_first(u64 n_bits, u64 batch, u64 g, const u64 *const *mask, u64 n_mask, const u64 *s, u64 w,
                      const u64 *const *values, const u64 *t, u64 *const *out, u64 *any, u64 n_labels,
                      const u64 *labels, const u64 *label_bits, u64 *const *label_out, hipStream_t stream);

// the (slot + 1)-th row whose encrypted mask bit is set (csgn_uint_nth.hip), include/csgn_hip.h's definition: G_{r,s} the
// sum over d in s..r with C(d, s) odd and the d-subsets of the rows below r, lexicographic, of m_{i_1} * ... * m_{i_d} *
// m_r; output j the sum, ascending in r, of G_{r,s} * d_{r,j}, valid that of G_{r,s}, label plane i that of the G_{r,s}
// whose public label has bit label_bits[i].  mask: one grouped batch (n_mask == 1) or g batches of `batch` elements,
// every row of tm terms; values: w = 0..64 grouped planes, terms t[j]; valid, label_out: nullptr / n_labels == 0 = not
// written.
constexpr u32 kNthMaxGroup = 64, kNthMaxPlanes = 64, kNthMaxLabels = 64;
u64 uint_nth_terms(u64 g, u64 t, u64 slot, u64 row);    // P_{row,slot}, Q_slot for row == g; 0: invalid or 2^62 or more
u64 uint_nth_label_terms(u64 g, u64 t, u64 slot, const u64 *labels, u64 bit);   // 0 also where no row >= slot has the bit
hipError_t uint_nth(u64 n_bits, u64 batch, u64 g, u64 slot, const u64 *const *mask, u64 n_mask, u64 tm, u64 w,
                    const u64 *const *values, const u64 *t, u64 *const *out, u64 *valid, u64 n_labels, const u64 *labels,
                    const u64 *label_bits, u64 *const *label_out, hipStream_t stream);

// the product of two encrypted bit matrices over F2 (csgn_matmul.hip), include/csgn_hip.h's definition: C[i,k] is the
// sum, ascending in e < inner, of A[i,e] * B[e,k].  A: rows * inner elements of ta terms, B: inner * cols elements of
// tb terms (transposed: element k * inner + e), C: rows * cols elements of inner * ta * tb terms.
u64 matmul_terms(u64 inner, u64 ta, u64 tb);   // 0: a zero argument or a count of 2^62 or more
const char *matmul_kernel_name(u64 n_bits, u64 rows, u64 inner, u64 cols, u64 ta, u64 tb, bool transposed);
hipError_t matmul(u64 n_bits, u64 rows, u64 inner, u64 cols, const u64 *A, u64 ta, const u64 *B, u64 tb,
                  bool transposed, u64 *C, hipStream_t stream);

// encrypted bits counted into encrypted integers (csgn_count.hip), include/csgn_hip.h's definition: plane j of element q
// is the sum, over the 2^j-subsets of the element's `group` inputs in lexicographic order, of the products of the
// subset's inputs.  in: one grouped batch (n_in == 1) or `group` batches of `count` elements; js: n_out strictly
// ascending planes; out[x]: count * count_terms(group, t, js[x]) * dL words.
u64 count_terms(u64 group, u64 t, u64 j);      // 0: a zero argument, j > 6, 2^j > group or a count of 2^62 or more
bool count_shape_ok(u64 count, u64 group, u64 t, u64 n_in, u64 n_out, const u64 *js);   // the arguments, sizes apart
const char *count_kernel_name(u64 n_bits, u64 count, u64 group, u64 t, u64 n_in, u64 n_out, const u64 *js);
hipError_t count(u64 n_bits, u64 count, u64 group, u64 t, const u64 *const *in, u64 n_in, u64 n_out, const u64 *js,
                 u64 *const *out, hipStream_t stream);

// running counts of encrypted bits (csgn_count_prefix.hip), include/csgn_hip.h's definition: row r of plane j is count's
// plane j of the element's first r + 1 - exclusive inputs, or the one ZERO term where 2^j passes them; out[x]: the rows
// one after the other, row r `count` elements from term count * count_prefix_offset(.., r) on.
u64 count_prefix_offset(u64 group, u64 t, u64 j, u64 exclusive, u64 r);   // r = group: A_j; 0: invalid or 2^62 or more
bool count_prefix_shape_ok(u64 count, u64 group, u64 t, u64 exclusive, u64 n_in, u64 n_out, const u64 *js);
hipError_t count_prefix(u64 n_bits, u64 count, u64 group, u64 t, u64 exclusive, const u64 *const *in, u64 n_in,
                        u64 n_out, const u64 *js, u64 *const *out, hipStream_t stream);

// encrypted integers summed into encrypted integers (csgn_wsum.hip), include/csgn_hip.h's definition: class c holds n_c
// ciphertexts of weight 2^c and of t terms each; plane j of an element is the sum, over the count vectors (m_j .. m_0)
// with sum m_c 2^c = 2^j in ascending order and over their selections (class j slowest), of the products of the selected
// inputs, classes descending.  A plan compiles the vectors of the requested planes for one (n_c, t); it lives in a
// csgn_wsum_plan object of the caller's.
constexpr u32 kWsumMaxClasses = 64, kWsumMaxPlane = 62, kWsumMaxPlanes = 63;
constexpr u64 kWsumMaxInputs = 65536, kWsumMaxVectors = 65536;
struct WsumPlan {
    u32 C = 0, n_out = 0;
    u64 t = 0;
    u32 n[kWsumMaxClasses] = {};
    u32 js[kWsumMaxPlanes] = {};
    u64 T[kWsumMaxPlanes] = {};         // terms per element of plane js[x]
    u32 ncls[kWsumMaxPlanes] = {};      // classes 0 .. ncls - 1 take part in plane js[x]
    u32 nvec[kWsumMaxPlanes] = {}, vbase[kWsumMaxPlanes] = {}, parts[kWsumMaxPlanes] = {};
    u64 max_part = 0;                   // terms of the largest part
    u32 sub_bytes = 0;                  // bytes of member indices of the largest part
    u32 *d_vt = nullptr;                // the vector table (csgn_wsum.hip)
    std::vector<u32> vt;                // its host copy
};
u64 wsum_terms(u64 n_classes, const u64 *n, u64 t, u64 j);   // 0: a bad argument, an empty plane or 2^62 terms or more
// the arguments of a plan and T[x] of every plane: CSGN_ERR_INVALID (an empty plane among them), else
// CSGN_ERR_UNSUPPORTED when a plane reaches 2^31 terms
int wsum_plan_check(u64 n_classes, const u64 *n, u64 t, u64 n_out, const u64 *js, u64 *T);
// after wsum_plan_check: enumerates and uploads (synchronous); CSGN_ERR_UNSUPPORTED past kWsumMaxVectors vectors or
// for a monomial of more than 3072 factors
int wsum_plan_create(u64 n_classes, const u64 *n, u64 t, u64 n_out, const u64 *js, WsumPlan &p, hipError_t &herr);
void wsum_plan_free(WsumPlan &p);
hipError_t wsum(const WsumPlan &p, u64 n_bits, u64 count, const u64 *const *in, u64 *const *out, hipStream_t stream);

// selection by an encrypted comparison (csgn_uint_lt_select.hip), include/csgn_hip.h's definition: output i is
// (L * (X_i + Y_i)) + Y_i with L = lessThan(a, b), the LT_FIRST / LT_STEP chain.  a and b: w = 1..16 planes, terms ta[j] /
// tb[j]; requests: n_out = 0..64 pairs of planes, terms tx[i] / ty[i]; less: nullptr = not written (then n_out >= 1).
constexpr u32 kLtSelMaxWidth = 16, kLtSelMaxOut = 64;
u64 uint_lt_terms(u64 w, const u64 *ta, const u64 *tb);   // L; 0: invalid argument or a count of 2^62 or more
const char *uint_lt_select_kernel_name(u64 n_bits, u64 batch, u64 w, const u64 *ta, const u64 *tb, u64 n_out,
                                       const u64 *tx, const u64 *ty, bool less);
hipError_t uint_lt_select(u64 n_bits, u64 batch, u64 w, const u64 *const *a, const u64 *ta, const u64 *const *b,
                          const u64 *tb, u64 n_out, const u64 *const *x, const u64 *tx, const u64 *const *y,
                          const u64 *ty, u64 *const *out, u64 *less, hipStream_t stream);

// a + b, a - b, a == b, a != b of two encrypted integers (csgn_uint_arith.hip), include/csgn_hip.h's definition: the
// ADD_HALF / ADD_FULL and XNOR / EQ_STEP chains of csgn_uint_step; op = CSGN_UINT_ARITH_*.  a and b: w = 1..16 planes,
// terms ta[j] / tb[j]; out: w planes (EQ / NE: one); carry: the carry out of the top plane, nullptr = not computed.
constexpr u32 kArithMaxWidth = 16;
u64 uint_arith_terms(int op, u64 w, const u64 *ta, const u64 *tb, u64 output);   // 0: invalid argument or 2^62 or more
const char *uint_arith_kernel_name(u64 n_bits, int op, u64 batch, u64 w, const u64 *ta, const u64 *tb, bool carry);
hipError_t uint_arith(u64 n_bits, int op, u64 batch, u64 w, const u64 *const *a, const u64 *ta, const u64 *const *b,
                      const u64 *tb, u64 *const *out, u64 *carry, hipStream_t stream);

// a + (s ? k : 0) of an encrypted integer, an encrypted flag and a public constant (csgn_uint_add_where.hip),
// include/csgn_hip.h's definition: uint_arith's ADD chain with b_j = s where k_j = 1 and no b_j where k_j = 0.  a: w =
// 1..32 planes, terms ta[j]; sel: one batch of ts terms (may be null for k = 0); out: w planes; carry: nullptr = not
// computed.
constexpr u32 kAddWhereMaxWidth = 32;
bool uint_add_where_terms(u64 w, u64 k, u64 ts, const u64 *ta, u64 *T);   // T[0..w]; false: invalid or 2^62 or more
u64 uint_add_where_output_terms(u64 w, u64 k, u64 ts, const u64 *ta, u64 output);   // 0: invalid or 2^62 or more
hipError_t uint_add_where(u64 n_bits, u64 batch, u64 w, u64 k, const u64 *sel, u64 ts, const u64 *const *a,
                          const u64 *ta, u64 *const *out, u64 *carry, hipStream_t stream);

// a & b, a | b, a ^ b, ~a, select(s, a, b) and s * a of encrypted integers, plane by plane (csgn_uint_bitwise.hip),
// include/csgn_hip.h's definition; op = CSGN_UINT_BITWISE_*.  a and b: w = 1..64 planes, terms ta[j] / tb[j]; sel: one
// batch of ts terms; out: w planes.  Operands the op does not read: their counts are ignored, their pointers may be null.
constexpr u32 kBitwiseMaxPlanes = 64;
u64 uint_bitwise_terms(int op, u64 ts, u64 ta, u64 tb);   // 0: unknown op, a zero count that is read, or 2^62 or more
const char *uint_bitwise_kernel_name(u64 n_bits, int op, u64 batch, u64 w, u64 ts, const u64 *ta, const u64 *tb);
hipError_t uint_bitwise(u64 n_bits, int op, u64 batch, u64 w, const u64 *sel, u64 ts, const u64 *const *a, const u64 *ta,
                        const u64 *const *b, const u64 *tb, u64 *const *out, hipStream_t stream);

// a public matrix over F2 applied to an encrypted integer (csgn_uint_linear.hip), include/csgn_hip.h's definition:
// output j is the left-nested sum, ascending in i, of the input planes bit i of rows[j] names, then ONE where bit j of
// `constant` is set; a zero row is the one-term constant.  in: nin = 1..64 planes, terms ta[i]; out: nout = 1..64 planes.
constexpr u32 kLinearMaxPlanes = 64;
u64 uint_linear_terms(u64 nin, const u64 *ta, u64 row, int constant_bit);   // 0: invalid or 2^62 or more
// the input plane and term output term q of a row copies (plane nin: ONE, nin + 1: ZERO); false: invalid or q past the row
bool uint_linear_decode(u64 nin, const u64 *ta, u64 row, int constant_bit, u64 q, u64 *plane, u64 *term);
// plan[8]: unit bytes for 16-byte-aligned pointers, units per element, G, tiles, workgroups per tile, launches under the
// calling thread's launch_blocks, the tile budget in units, plane groups; false: an invalid shape
bool uint_linear_plan(u64 n_bits, u64 batch, u64 nin, const u64 *ta, u64 nout, const u64 *rows, u64 constant, u64 *plan);
hipError_t uint_linear(u64 n_bits, u64 batch, u64 nin, const u64 *const *in, const u64 *ta, u64 nout, const u64 *rows,
                       u64 constant, u64 *const *out, hipStream_t stream);

// sums of comparisons of one encrypted integer against public constants (csgn_uint_plain_sum.hip), include/csgn_hip.h's
// definition: output plane x is the left-nested sum of the csgn_uint_plain results of its entries
// (cmp[i], k[i]), first[x] <= i < first[x + 1], then ONE where bit x of `constant` is set; a plane of no entry is the
// one-term constant.  A plan holds the shape and, on the device, every entry's level record; it lives in a
// csgn_uint_plain_sum_plan object of the caller's.
constexpr u32 kPlainSumMaxPlanes = 64;
constexpr u64 kPlainSumMaxEntries = 65536;
struct PlainSumPlan {
    u32 w = 0, n_out = 0, stride = 0;   // input planes, output planes, words of a record
    u64 constant = 0;
    u64 t[64] = {};                     // terms per element of input plane j
    u64 T[kPlainSumMaxPlanes] = {};     // terms per element of output plane x
    u32 runs[kPlainSumMaxPlanes] = {};  // its runs of up to 16 terms, the constant's included
    u32 efirst[kPlainSumMaxPlanes + 1] = {};
    std::vector<u32> rec;               // the records' host copy
    u32 *d_rec = nullptr;
};
// T of one plane; 0: an argument csgn_uint_plain_terms refuses, a null array, a constant_bit other than 0 / 1 or 2^62
u64 uint_plain_sum_terms(u64 width, const u64 *terms, u64 n_entries, const int *cmp, const u64 *k, int constant_bit);
// the factors of term q of one plane as (plane, term) pairs (plane width: ONE, width + 1: ZERO); false: refused, q past
// the plane, more than kPlainSumMaxEntries entries or a plane of 2^31 terms or more
bool uint_plain_sum_decode(u64 width, const u64 *terms, u64 n_entries, const int *cmp, const u64 *k, int constant_bit,
                           u64 q, u64 *level_plane, u64 *level_term, u64 *n_factors);
// the shape of a plan (host only; records: with the level records): CSGN_ERR_INVALID, else CSGN_ERR_UNSUPPORTED past
// kPlainSumMaxEntries entries or for a plane of 2^31 terms or more
int uint_plain_sum_shape(u64 width, const u64 *terms, u64 n_out, const u64 *first, const int *cmp, const u64 *k,
                         u64 constant, bool records, PlainSumPlan &pl);
int uint_plain_sum_create(PlainSumPlan &pl, hipError_t &herr);   // uploads the records (synchronous); CSGN_ERR_HIP
void uint_plain_sum_free(PlainSumPlan &pl);
// plan[6]: unit bytes for 16-byte-aligned pointers, lane items per element, plane groups, launches under the calling
// thread's launch_blocks, elements and workgroups of the first launch
void uint_plain_sum_plan(const PlainSumPlan &pl, u64 n_bits, u64 batch, u64 *plan);
hipError_t uint_plain_sum(const PlainSumPlan &pl, u64 n_bits, u64 batch, const u64 *const *planes, u64 *const *out,
                          hipStream_t stream);

// a public bilinear form over F2 of two encrypted integers (csgn_uint_bilinear.hip), include/csgn_hip.h's definition:
// output plane x is the left-nested sum of the products a_left[i] * b_right[i] of its entries, first[x] <= i <
// first[x + 1], then ONE where bit x of `constant` is set; a plane of no entry is the one-term constant.  A plan holds
// the shape and, on the device, the plane tables and every entry's first term and pair; it lives in a
// csgn_uint_bilinear_plan object of the caller's.
constexpr u32 kBilinearMaxPlanes = 64;
constexpr u64 kBilinearMaxEntries = 262144;
struct BilinearPlan {
    u32 wa = 0, wb = 0, n_out = 0;
    bool eq = false;                    // every ta equal, every tb equal, ta * tb below 2^31: the entry by division
    u64 constant = 0;
    u64 ta[kBilinearMaxPlanes] = {}, tb[kBilinearMaxPlanes] = {};   // terms per element of the input planes
    u64 T[kBilinearMaxPlanes] = {};     // terms per element of output plane x
    u32 efirst[kBilinearMaxPlanes + 1] = {};
    std::vector<u32> start, lr;         // per entry: its first term in its plane; left | right << 8
    void *d_tab = nullptr;
};
// T of one plane; 0: a width outside 1..64, a null array, a plane of 0 terms, an index at or past its width, a
// constant_bit other than 0 / 1 or 2^62 terms or more
u64 uint_bilinear_terms(u64 wa, const u64 *ta, u64 wb, const u64 *tb, u64 n_entries, const u64 *left, const u64 *right,
                        int constant_bit);
// the entry and the (left, right) terms of term q of one plane (entry n_entries: ONE, n_entries + 1: ZERO); false:
// refused, q past the plane, more than kBilinearMaxEntries entries or a plane of 2^31 terms or more
bool uint_bilinear_decode(u64 wa, const u64 *ta, u64 wb, const u64 *tb, u64 n_entries, const u64 *left, const u64 *right,
                          int constant_bit, u64 q, u64 *entry, u64 *left_term, u64 *right_term);
// the shape of a plan (host only): CSGN_ERR_INVALID, else CSGN_ERR_UNSUPPORTED past kBilinearMaxEntries entries or for
// a plane of 2^31 terms or more
int uint_bilinear_shape(u64 wa, const u64 *ta, u64 wb, const u64 *tb, u64 n_out, const u64 *first, const u64 *left,
                        const u64 *right, u64 constant, BilinearPlan &pl);
int uint_bilinear_create(BilinearPlan &pl, hipError_t &herr);   // uploads the tables (synchronous); CSGN_ERR_HIP
void uint_bilinear_free(BilinearPlan &pl);
// plan[12]: unit bytes for 16-byte-aligned pointers, units per element, G, tiles, workgroups per tile, launches under
// the calling thread's launch_blocks, workgroups of the first launch, plane groups, staged, units a workgroup walks,
// operand units per element, the LDS budget in bytes
void uint_bilinear_launches(const BilinearPlan &pl, u64 n_bits, u64 batch, u64 *plan);
hipError_t uint_bilinear(const BilinearPlan &pl, u64 n_bits, u64 batch, const u64 *const *a, const u64 *const *b,
                         u64 *const *out, hipStream_t stream);

// a public polynomial over F2 of encrypted planes (csgn_uint_poly.hip), include/csgn_hip.h's definition: output plane x
// is the left-nested sum of its monomials, mfirst[x] <= m < mfirst[x + 1], each the left-nested product of 1 to 8
// input planes, then ONE where bit x of `constant` is set; a plane of no monomial is the one-term constant.  A plan
// holds the shape and, on the device, the plane tables and one 16-byte record per monomial; it lives in a
// csgn_uint_poly_plan object of the caller's.
constexpr u32 kPolyMaxIn = 256;
constexpr u32 kPolyMaxOut = 64;
constexpr u32 kPolyMaxDegree = 8;
constexpr u64 kPolyMaxMonomials = 262144;
struct PolyPlan {
    u32 n_in = 0, n_out = 0;
    bool teq = false;                   // every input plane has tin[0] terms, below 2^31
    bool eq = false;                    // teq, and every monomial has degree `deg`, tin[0]^deg below 2^31: the monomial by division
    u32 deg = 0;
    u64 constant = 0;
    u64 tin[kPolyMaxIn] = {};           // terms per element of the input planes
    u64 T[kPolyMaxOut] = {};            // terms per element of output plane x
    u32 mfirst[kPolyMaxOut + 1] = {};
    std::vector<u32> rec;               // per monomial, four words: its first term in its plane, its degree, its
                                        // factors one byte each (the first factor in the low byte of word 2)
    void *d_tab = nullptr;
};
// T of one plane whose monomial m has the factors factor[mfirst[m] .. mfirst[m + 1] - 1]; 0: n_in outside 1..256, a
// null array, a plane of 0 terms, a degree outside 1..8, a factor at or past n_in, a constant_bit other than 0 / 1 or
// 2^62 terms or more
u64 uint_poly_terms(u64 n_in, const u64 *terms, u64 n_monomials, const u64 *mfirst, const u64 *factor, int constant_bit);
// the monomial and the factors' term indices (8 values, 0 past the degree) of term q of one plane (monomial
// n_monomials: ONE, n_monomials + 1: ZERO); false: refused, q past the plane, more than kPolyMaxMonomials monomials or
// a plane of 2^31 terms or more
bool uint_poly_decode(u64 n_in, const u64 *terms, u64 n_monomials, const u64 *mfirst, const u64 *factor, int constant_bit,
                      u64 q, u64 *monomial, u64 *factor_terms);
// the shape of a plan (host only): CSGN_ERR_INVALID, else CSGN_ERR_UNSUPPORTED past kPolyMaxMonomials monomials or for a
// plane of 2^31 terms or more
int uint_poly_shape(u64 n_in, const u64 *terms, u64 n_out, const u64 *first, const u64 *mfirst, const u64 *factor,
                    u64 constant, PolyPlan &pl);
int uint_poly_create(PolyPlan &pl, hipError_t &herr);   // uploads the tables (synchronous); CSGN_ERR_HIP
void uint_poly_free(PolyPlan &pl);
// plan[14]: unit bytes for 16-byte-aligned pointers, units per element, G, tiles, workgroups per tile, launches under
// the calling thread's launch_blocks, workgroups of the first launch, plane groups, staged, units a workgroup walks,
// operand units per element, the LDS budget in bytes, the monomial by division (eq), the factor terms' mode (0: every
// plane has one term, 1: one shared divisor, 2: a divisor per plane)
void uint_poly_launches(const PolyPlan &pl, u64 n_bits, u64 batch, u64 *plan);
hipError_t uint_poly(const PolyPlan &pl, u64 n_bits, u64 batch, const u64 *const *in, u64 *const *out, hipStream_t stream);

// an encrypted integer shifted, rotated or indexed by an encrypted amount (csgn_uint_pick.hip), include/csgn_hip.h's
// definition: output j is the sum, ascending in r < rows_j, of EQ(index, r) * a_{src(j, r)}; op = CSGN_UINT_PICK_*.
// index planes: v = 1..16, terms s[k]; source planes: w = 1..64, every one of t terms; rows: EACH's n, else 0.
constexpr u32 kPickMaxIndex = 16, kPickMaxPlanes = 64;
u64 uint_pick_terms(int op, u64 v, const u64 *s, u64 w, u64 rows, u64 j);   // E_j; 0: invalid argument or 2^62 or more
const char *uint_pick_kernel_name(u64 n_bits, int op, u64 batch, u64 v, const u64 *s, u64 w, u64 rows, u64 t);
// the fused form's tile: plan = {G, KC, QP, q parts}; wide: 16-byte units where dL is even.  false: invalid shape
bool uint_pick_plan(u64 n_bits, int op, u64 batch, u64 v, const u64 *s, u64 w, u64 rows, u64 t, bool wide, u64 plan[4]);
hipError_t uint_pick(u64 n_bits, int op, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 w, u64 rows,
                     const u64 *const *src, u64 t, u64 *const *out, hipStream_t stream);
// EACH over arrays whose row r has T[r] terms (include/csgn_hip.h, csgn_uint_pick_rows_offsets; host only): src_off /
// out_off get the rows + 1 term offsets of the rows in an array and of their blocks in an output element.  false: an
// invalid shape or a count of 2^62 or more
bool uint_pick_rows_offsets(u64 v, const u64 *s, u64 rows, const u64 *T, u64 *src_off, u64 *out_off);
// that read in one launch (csgn_uint_pick_rows.hip), include/csgn_hip.h's definition.  T: w * rows counts, plane-major.
// A[j] / Tout[j] of every plane (host only); false: an invalid shape or a count of 2^62 or more
bool uint_pick_rows_sizes(u64 v, const u64 *s, u64 rows, u64 w, const u64 *T, u64 *A, u64 *Tout);
const char *uint_pick_rows_kernel_name();       // of a valid shape under the calling thread's knob
// (r, in, c) of output position `position` by the kernel's own search and division (host only); a csgn_status
int uint_pick_rows_decode(u64 v, const u64 *s, u64 rows, const u64 *T, u64 position, u64 out[3]);
// the calling thread's row tables (host only): {tables kept, device copies retired, device copies freed}.  A copy that a
// capturing stream has used is retired, not freed, when its table leaves the cache or the device changes.
void uint_pick_rows_stats(u64 out[3]);
hipError_t uint_pick_rows(u64 n_bits, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 rows, u64 w,
                          const u64 *const *arrays, const u64 *T, u64 *const *out, hipStream_t stream);

// encrypted arrays written at encrypted indices (csgn_uint_write.hip), include/csgn_hip.h's definition: row r of element
// e's array in plane j becomes (EQ(index_e, r) * (value_{e,j} + d_{e*n+r,j})) + d_{e*n+r,j}.  index planes: v = 1..16,
// terms s[k]; value planes: w = 1..64, terms tv[j]; array planes: batch * rows elements, terms td[j].
constexpr u32 kWriteMaxIndex = 16, kWriteMaxPlanes = 64;
// the term offset of row r <= rows inside its array (r = rows: the array's terms A); 0: invalid argument or 2^62 or more
u64 uint_write_offset(u64 v, const u64 *s, u64 rows, u64 r, u64 tv, u64 td);
const char *uint_write_kernel_name(u64 n_bits, u64 batch, u64 v, const u64 *s, u64 rows, u64 w, const u64 *tv,
                                   const u64 *td);
// the fused form's tile: plan = {G, KC, QP, q parts}; wide: 16-byte units where dL is even.  false: invalid shape
bool uint_write_plan(u64 n_bits, u64 batch, u64 v, const u64 *s, u64 rows, u64 w, const u64 *tv, const u64 *td,
                     bool wide, u64 plan[4]);
hipError_t uint_write(u64 n_bits, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 rows, u64 w,
                      const u64 *const *value, const u64 *tv, const u64 *const *arrays, const u64 *td, u64 *const *out,
                      hipStream_t stream);

// The temporaries of the composed forms and of the gather plan (csgn_scratch.cpp): a plain (hipMalloc) block the calling
// thread keeps per stream and per user, never the stream-ordered pool.  Returns the block, or nullptr with e set
// (hipErrorStreamCaptureUnsupported when the call would have to allocate while s is capturing).  owned: the block is
// past the kept size and belongs to this call; scratch_done frees it behind the call's launches (waits for the device)
// and passes e through.  A kept block handed out while s is capturing is never freed before the thread ends: where
// growth or eviction would free it, it is retired instead, so a graph that holds it stays replayable.  Eviction (a
// ninth stream in one slot) takes the block used least recently.  scratch_stats: the calling thread's {blocks kept,
// bytes kept, blocks retired, hipMalloc calls of scratch_take, hipFree calls of scratch_take and scratch_done}.
enum ScratchSlot { SCRATCH_UINT_PLAIN, SCRATCH_UINT_LUT, SCRATCH_UINT_READ, SCRATCH_UINT_ADDK, SCRATCH_UINT_FIND, SCRATCH_GATHER, SCRATCH_MATMUL, SCRATCH_COUNT, SCRATCH_UINT_LT_SELECT, SCRATCH_UINT_PICK, SCRATCH_UINT_WRITE, SCRATCH_UINT_ARITH, SCRATCH_UINT_PICK_ROWS, SCRATCH_SLOTS };
u64 *scratch_take(ScratchSlot slot, size_t bytes, hipStream_t s, bool &owned, hipError_t &e);
hipError_t scratch_done(u64 *block, bool owned, hipError_t e);
void scratch_stats(u64 out[5]);

hipError_t small_ops(u64 n_bits, u64 count, const ::csgn_small_op *ops, hipStream_t s);
size_t decrypt_scratch_bytes(u64 batch, u64 total_terms);
// out[i] = a[i] & b[i] (is_product) or a[i] ^ b[i]: Dec(a*b) = Dec(a) & Dec(b), Dec(a+b) = Dec(a) ^ Dec(b)
hipError_t combine_bits(const uint8_t *a, const uint8_t *b, u64 n, bool is_product, uint8_t *out, hipStream_t s);
size_t decrypt_combined_scratch_bytes(u64 batch, u64 t1, u64 t2);
hipError_t decrypt_combined(u64 n_bits, u64 batch, u64 t1, u64 t2, const u64 *L, const u64 *R,
                            const u64 *mask, bool is_product, uint8_t *bits, void *scratch, hipStream_t s);

// n_planes = 1..64 one-bit batches decrypted into one word per element (csgn_uint_decrypt.hip), include/csgn_hip.h's
// definition: bit j of values[e] = Dec(element e of plane j).  terms[j]: plane j's terms per element, 0 = ragged; a
// ragged plane j has CSR offsets off[j] (device, batch + 1) and a bound max_terms[j] <= kLongTerms on one element's
// terms (off and max_terms may be nullptr when no plane is ragged).  No scratch.
constexpr u32 kUintDecryptMaxPlanes = 64;
// "k_uint_decrypt", "k_zero_words+k_uint_decrypt" (some uniform plane is cut into chunks), "": invalid shape
const char *uint_decrypt_kernel_name(u64 n_bits, u64 batch, u64 n_planes, const u64 *terms);
hipError_t uint_decrypt(u64 n_bits, u64 batch, u64 n_planes, const u64 *const *planes, const u64 *terms,
                        const u64 *const *off, const u64 *max_terms, const u64 *mask, u64 *values, hipStream_t stream);

} // namespace csgn
