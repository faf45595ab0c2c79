/*
 * csgn_hip.h -- C ABI of libcsgn_hip.so: the MI355X (gfx950) implementation of the
 * certFHE/CSGN ciphertext-arithmetic hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI layer; its seam is the set of
 * six private array functions behind the certFHE:: classes:
 *
 *   Ciphertext::defaultN_multiply   /root/reference/src/Ciphertext.cpp:124-131
 *   Ciphertext::multiply            /root/reference/src/Ciphertext.cpp:133-179
 *   Ciphertext::add                 /root/reference/src/Ciphertext.cpp:107-122
 *   SecretKey::encrypt(bit,n,d,s)   /root/reference/src/SecretKey.cpp:35-80   (+ packing :153-206)
 *   SecretKey::defaultN_decrypt     /root/reference/src/SecretKey.cpp:82-102
 *   SecretKey::decrypt(v,len,..)    /root/reference/src/SecretKey.cpp:104-147
 *
 * Each entry point below names the one(s) it replaces.  The certFHE:: C++ classes in
 * include/certfhe/ are implemented on top of exactly these symbols; INTEGRATION.md shows
 * the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - POD arguments only.  `const uint64_t *d_x` is a DEVICE pointer (HBM); `h_x` is a host
 *     pointer.  Nothing here allocates memory the caller must free with delete[].
 *   - Term buffers: a ciphertext of T terms at N bits is T*dL consecutive uint64 words,
 *     dL = ceil(N/64); bit j of a term is word j/64, bit 63-(j%64) (MSB first); the unused
 *     low bits of a term's last word are zero (src/Ciphertext.h:19-21, SecretKey.cpp:175-197).
 *     The reference's parallel `bitlen` array is a pure function of (N, T) for every
 *     ciphertext produced by encrypt/+/x and is NOT materialised on the device; see
 *     csgn_bitlen_canonical().
 *   - Batches: "uniform" = B ciphertexts of the same term count laid back to back;
 *     "ragged" = CSR: d_off[B+1] term offsets into one flat term buffer (empty ciphertexts
 *     allowed).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Compute calls
 *     are asynchronous on that stream; the caller synchronises.
 *   - Every function returns CSGN_OK (0) or a negative csgn_status; csgn_last_error() gives
 *     a thread-local message.  The reference has no error convention at all;
 *     misuse that is UB there is a reported error here.
 *   - Thread safety: no hidden global state except per-thread items: the error string, the
 *     tuning knobs, the ragged planner's small device scratch, the temporary blocks of the
 *     composed forms and of csgn_gather_plan (one per user and stream, at most 8 streams per
 *     user, the least recently used evicted; csgn_uint_addk has the rules) and the row tables of
 *     csgn_uint_pick_rows (up to 128, least recently used evicted).  A thread's device memory is
 *     returned when the thread ends; csgn_scratch_stats reports it.  One host thread (or
 *     process) per GPU may call concurrently.
 *   - Graphs: a graph that captured a composed-form call or a csgn_uint_pick_rows call holds
 *     the capturing thread's temporary block or row table.  Such memory is never freed while
 *     that thread lives: where growth, eviction or a change of device would free it, it is
 *     retired instead and returned at thread exit.  The graph stays replayable for as long as
 *     the capturing thread lives, and no longer.
 *   - There is NO CPU fallback: without a gfx950 device every compute call fails with
 *     CSGN_ERR_NO_DEVICE.
 */
#ifndef CSGN_HIP_H
#define CSGN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum csgn_status {
    CSGN_OK = 0,
    CSGN_ERR_INVALID = -1,      /* bad argument (null pointer, N==0, key index >= N, ...) */
    CSGN_ERR_UNSUPPORTED = -2,  /* shape outside what the kernels handle (see each call) */
    CSGN_ERR_NO_DEVICE = -3,    /* no HIP device / not gfx950 */
    CSGN_ERR_HIP = -4           /* a HIP runtime call failed; message has the detail */
} csgn_status;

#define CSGN_ABI_VERSION 1

/* ------------------------------------------------------------------ runtime ---- */

int csgn_abi_version(void);
const char *csgn_last_error(void);

/* Select `device` for the calling thread and verify it is a gfx950 part. */
int csgn_init(int device);
int csgn_device_count(int *h_count);
/* Fills h_name (<= cap bytes) with the gcnArchName and reports CU count / HBM bytes. */
int csgn_device_info(int device, char *h_name, size_t cap, int *h_cu_count, uint64_t *h_hbm_bytes);

int csgn_malloc(void **d_ptr, size_t bytes);
int csgn_free(void *d_ptr);
/* Pinned host memory the GPU can address: *h_ptr for the host, *d_alias for kernels (results
 * a kernel writes there are visible to the host after csgn_stream_sync, no copy).  Used by the
 * C++ classes for the one-byte answer of SecretKey::decrypt. */
int csgn_host_alloc(void **h_ptr, void **d_alias, size_t bytes);
int csgn_host_free(void *h_ptr);
/* Host-buffer lifetime: h_src / h_dst belong to the call until `stream` has passed the copy.  From or to
 * pageable memory the runtime happens to stage the copy before it returns, but that is not part of this
 * contract: synchronise the stream (or use csgn_host_alloc memory that outlives it) before freeing or
 * reusing the buffer. */
int csgn_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream);
int csgn_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream);
int csgn_memcpy_d2d(void *d_dst, const void *d_src, size_t bytes, void *stream);
int csgn_memset(void *d_dst, int value, size_t bytes, void *stream);
int csgn_stream_create(void **stream);
int csgn_stream_destroy(void *stream);
int csgn_stream_sync(void *stream);
int csgn_event_create(void **event);
int csgn_event_destroy(void *event);
int csgn_event_record(void *event, void *stream);
int csgn_event_elapsed_ms(void *start, void *stop, float *h_ms);   /* synchronises on stop */
int csgn_event_sync(void *event);                                  /* returns once the work recorded in front of the event has run */

/* ------------------------------------------------- host-side metadata helpers ---- */

/* Context::getDefaultN, src/Context.cpp:24-28. */
uint64_t csgn_default_len(uint64_t n_bits);
/* Context S = N/(2D), src/Context.cpp:22. */
uint64_t csgn_context_s(uint64_t n_bits, uint64_t d);
/* Result length in words of Ciphertext::multiply, src/Ciphertext.cpp:135-146. */
uint64_t csgn_mul_len(uint64_t n_bits, uint64_t len1, uint64_t len2);
/* The bitlen side-array the reference would hold for a T-term ciphertext
 * (src/SecretKey.cpp:171-173 per term): h_bitlen[T*dL]. */
int csgn_bitlen_canonical(uint64_t n_bits, uint64_t terms, uint64_t *h_bitlen);
/* Pack a secret key (D indices in [0,N), src/SecretKey.h:22) into the dL-word MSB-first
 * mask the decrypt/encrypt kernels consume.  Duplicate indices are allowed (setKey does
 * not forbid them, src/SecretKey.cpp:292-302); an index >= N is CSGN_ERR_INVALID. */
int csgn_key_mask(uint64_t n_bits, const uint64_t *h_key, uint64_t d, uint64_t *h_mask);

/* ------------------------------------------------------------------ multiply ---- */

/* Batched Ciphertext::multiply (src/Ciphertext.cpp:133-179) incl. the 1x1 fast path
 * defaultN_multiply (:124-131).  For every pair b < batch:
 *     out_b[(i*t2 + j)*dL + k] = L_b[i*dL + k] & R_b[j*dL + k]      i<t1, j<t2, k<dL
 * d_left: batch*t1*dL words, d_right: batch*t2*dL, d_out: batch*t1*t2*dL.
 * Pair p's product goes to slot (p % out_slots) of d_out when out_slots != 0 (streaming a
 * batch through a fixed arena, SURVEY 8d "streaming rule"); out_slots == 0 means one slot
 * per pair.  With out_slots < batch the call is split into launches of <= out_slots pairs
 * in stream order so later pairs overwrite earlier ones deterministically.
 * Limits: dL*8 <= 16384 bytes per term; t1*t2*dL < 2^32 per pair.
 * The kernel is chosen per shape (csgn_mul_uniform_kernel names it): calls with >= 4 MB of
 * operands whose output is >= 4x the operands are preceded by a read-only pass over the
 * operands that leaves them in the GPU's memory-side cache, so the operands are READ twice;
 * nothing but d_out is written. */
int csgn_mul_uniform(uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2,
                     const uint64_t *d_left, const uint64_t *d_right, uint64_t *d_out,
                     uint64_t out_slots, void *stream);

/* Ragged form.  Step 1 (plan): from the operand term offsets compute the product term
 * offsets d_off_out[batch+1] (exclusive scan of t1_b*t2_b) on the device and return
 * h_plan[0] = total output terms, h_plan[1] = max t1, h_plan[2] = max t2,
 * h_plan[3] = max t1*t2.  Synchronises `stream`.  d_off_out doubles as the per-pair result
 * term counts the multi-GPU driver gathers (count_b = off[b+1]-off[b]). */
int csgn_mul_ragged_plan(uint64_t batch, const uint64_t *d_off_left, const uint64_t *d_off_right,
                         uint64_t *d_off_out, uint64_t h_plan[4], void *stream);
/* Step 2: the products, into d_out[h_plan[0]*dL] at the planned offsets; pass the plan's
 * max_t1 = h_plan[1], max_t2 = h_plan[2], total_out_terms = h_plan[0].  Nearly uniform batches
 * of large products run the LDS-tiled kernel, and so do batches of small pairs whose largest shape is
 * small too (one narrow workgroup per pair); a batch whose pairs ALL have the largest shape runs
 * the uniform kernels; skewed or small ones a flat kernel whose grid is the real output (a workgroup
 * finds its first pair by a 64-ary search over d_off_out and stages the offsets it needs in LDS).
 * A pure function of its arguments: it keeps no state from the plan call (round 3 did, per host thread;
 * what a plan knows beyond its four numbers now lives in a csgn_mul_plan object, below).  Through this
 * entry a skewed batch's huge pairs take the CSR kernel like everything else and a product above 1 GiB is
 * written in 1 GiB slices. */
int csgn_mul_ragged(uint64_t n_bits, uint64_t batch,
                    const uint64_t *d_left, const uint64_t *d_off_left,
                    const uint64_t *d_right, const uint64_t *d_off_right,
                    uint64_t *d_out, const uint64_t *d_off_out,
                    uint64_t max_t1, uint64_t max_t2, uint64_t total_out_terms, void *stream);

/* The same two steps with the plan kept in an OBJECT of the caller's (round 4; supersedes the round-3 rule that
 * csgn_mul_ragged found the last plan of the calling thread by array addresses).  csgn_mul_plan_ragged is
 * csgn_mul_ragged_plan and additionally notes in *plan the batch's HUGE pairs (24 MB of output and more, up to
 * 32 of them), its operand size and a checksum of the three offset arrays; csgn_mul_planned multiplies by that
 * plan: a huge pair gets a uniform launch of its own when such pairs are most of the batch, a product above
 * 1 GiB is written in slices sized from the operand size.  The offset arrays belong to the plan until the next
 * csgn_mul_plan_ragged on it.  Because a huge pair's launch uses host copies of its offsets, csgn_mul_planned
 * first CHECKS the offset arrays against the plan's checksum whenever it is about to use such records (one
 * small kernel and a stream synchronise) and returns CSGN_ERR_INVALID if they changed;
 * csgn_mul_plan_trust(plan, 1) turns that check off for a caller who guarantees it.
 * csgn_mul_plan_validate does the check on demand.  A plan is used by one host thread at a time. */
typedef struct csgn_mul_plan csgn_mul_plan;
int csgn_mul_plan_create(csgn_mul_plan **plan);
void csgn_mul_plan_destroy(csgn_mul_plan *plan);
int csgn_mul_plan_ragged(csgn_mul_plan *plan, uint64_t batch, const uint64_t *d_off_left,
                         const uint64_t *d_off_right, uint64_t *d_off_out, uint64_t h_plan[4], void *stream);
int csgn_mul_planned(csgn_mul_plan *plan, uint64_t n_bits, const uint64_t *d_left, const uint64_t *d_right,
                     uint64_t *d_out, void *stream);
int csgn_mul_plan_validate(csgn_mul_plan *plan, void *stream);     /* CSGN_ERR_INVALID: offsets changed since the plan */
int csgn_mul_plan_trust(csgn_mul_plan *plan, int trust);

/* Ragged multiply with NO host round trip: the plan kernel and the multiply are enqueued back to back and
 * nothing is read back.  d_off_out[batch+1] is written as by csgn_mul_ragged_plan.  The caller gives the room:
 * out_capacity_terms = terms d_out can hold (an upper bound on the sum of t1_b*t2_b, e.g. from static shapes);
 * the launch is sized for it and stops at the real end, which only the device knows.  If the products do
 * not fit, NOTHING is written and the result's fifth word says so.  d_plan: device block of
 * csgn_mul_ragged_async_plan_words(batch) words, valid until the stream has passed the call.
 * Kernels: the CSR kernel, or -- decided on the device -- the plain AND stream when every pair is 1 x 1; the
 * LDS-tiled and per-huge-pair forms need shapes on the host and belong to csgn_mul_planned.
 * csgn_mul_ragged_async_result (optional, synchronises): h_result[0..3] as h_plan of csgn_mul_ragged_plan,
 * h_result[4] = 1 if the products did not fit. */
uint64_t csgn_mul_ragged_async_plan_words(uint64_t batch);
int csgn_mul_ragged_async(uint64_t n_bits, uint64_t batch,
                          const uint64_t *d_left, const uint64_t *d_off_left,
                          const uint64_t *d_right, const uint64_t *d_off_right,
                          uint64_t *d_out, uint64_t *d_off_out, uint64_t out_capacity_terms,
                          uint64_t *d_plan, void *stream);
int csgn_mul_ragged_async_result(const uint64_t *d_plan, uint64_t h_result[5], void *stream);

/* ----------------------------------------------------------------------- add ---- */

/* Batched Ciphertext::add (src/Ciphertext.cpp:107-122): out_b = L_b || R_b, t1+t2 terms.
 * No XOR, no de-duplication -- exactly the reference. */
int csgn_add_uniform(uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2,
                     const uint64_t *d_left, const uint64_t *d_right, uint64_t *d_out,
                     void *stream);
/* Ragged: d_off_out[b] = d_off_left[b] + d_off_right[b] is written by the call;
 * total_terms_out = d_off_left[batch] + d_off_right[batch] (the caller sized d_out with it). */
int csgn_add_ragged(uint64_t n_bits, uint64_t batch,
                    const uint64_t *d_left, const uint64_t *d_off_left,
                    const uint64_t *d_right, const uint64_t *d_off_right,
                    uint64_t *d_out, uint64_t *d_off_out,
                    uint64_t total_terms_out, void *stream);
/* The same with the caller's bounds on the term counts of one element of either operand (0, 0 = unknown).  The
 * offsets are device data; the bounds are how a caller that knows its shapes -- a class layer that built the
 * batch, a circuit -- tells the dispatch: with batch * (max_t1 + max_t2) == total_terms_out every pair has exactly
 * max_t1 + max_t2 terms, no lane has to find its pair and the uniform kernel runs (a million 1+1 sums given as CSR:
 * 73 % of the HBM peak against 55 % through the CSR kernel).  d_off_out is written either way.  Bounds too small
 * for total_terms_out are refused; bounds that do not hold (an element with more terms than stated) are the caller's
 * error, as wrong offsets would be. */
int csgn_add_ragged_bounded(uint64_t n_bits, uint64_t batch, uint64_t max_t1, uint64_t max_t2,
                            const uint64_t *d_left, const uint64_t *d_off_left,
                            const uint64_t *d_right, const uint64_t *d_off_right,
                            uint64_t *d_out, uint64_t *d_off_out,
                            uint64_t total_terms_out, void *stream);

/* A LIST of small, independent operations in one launch (round 5).  BASELINE config 1 is single operations on
 * one- and two-term ciphertexts behind a value-semantic API (tests/basic_operations.cpp:26-40): 480 bytes of traffic
 * and 2-3 us of launch each when issued one by one, 10-20 x the reference's 0.12-0.28 us.  A caller that can QUEUE
 * such operations (the class layer does: csgn_amd/csrc/certfhe/runtime.cpp) hands the queue over as records
 *     out = left + right (kind 0: concatenation, src/Ciphertext.cpp:107-122) or left * right (kind 1: all-pairs AND,
 *     :146-163), t1 / t2 terms a side, one workgroup per record.
 * d_ops must be readable by the device: device memory, or pinned host memory through its device alias
 * (csgn_host_alloc) -- the records are then read over the link, no copy is enqueued.  The operations of ONE call
 * must not read one another's outputs (split dependent ones over calls: the stream orders them); the record array
 * must stay untouched until the launch has run.  Meant for small shapes (a workgroup walks its output): use the
 * uniform / ragged calls for anything large.  Words are those of csgn_add_uniform / csgn_mul_uniform. */
typedef struct csgn_small_op {
    const uint64_t *left;
    const uint64_t *right;
    uint64_t *out;
    uint32_t t1, t2;
    uint32_t kind;           /* 0 add, 1 multiply */
    uint32_t reserved;
} csgn_small_op;
int csgn_small_ops(uint64_t n_bits, uint64_t count, const csgn_small_op *d_ops, void *stream);

/* ------------------------------------------------------------------- decrypt ---- */

/* Batched SecretKey::decrypt (src/SecretKey.cpp:104-147; single term :82-102):
 *     bit_b = XOR over terms k of ( AND over key indices s of term_k[s] )
 * d_mask is the dL-word key mask (csgn_key_mask) in device memory; d_bits receives one
 * byte (0/1) per ciphertext.  d_scratch must hold csgn_decrypt_scratch_bytes(batch, total
 * terms) bytes (one hit bit per term + one partial-parity word per ciphertext).  An empty
 * ciphertext decrypts to 0, as in the reference. */
size_t csgn_decrypt_scratch_bytes(uint64_t batch, uint64_t total_terms);
int csgn_decrypt_uniform(uint64_t n_bits, uint64_t batch, uint64_t terms,
                         const uint64_t *d_terms, const uint64_t *d_mask,
                         uint8_t *d_bits, void *d_scratch, void *stream);
int csgn_decrypt_ragged(uint64_t n_bits, uint64_t batch, uint64_t total_terms,
                        const uint64_t *d_terms, const uint64_t *d_off, const uint64_t *d_mask,
                        uint8_t *d_bits, void *d_scratch, void *stream);
/* The same with what the caller knows about the shapes: max_terms = an upper bound on the terms of any ONE
 * ciphertext (0 = unknown: csgn_decrypt_ragged).  The offsets live on the device, so the bound is the only way the
 * dispatch can learn what a class layer or a circuit knows anyway: with batch * max_terms == total_terms every
 * ciphertext has exactly max_terms terms and the uniform kernels run (a million single-term ciphertexts handed over as
 * CSR: one kernel that writes the plaintext bytes itself, 76 % of the HBM peak against 60 % through the CSR passes); with
 * max_terms <= 4096 the launch that folds long ciphertexts chunk by chunk is not made.  A bound that is too small for
 * total_terms is refused (CSGN_ERR_INVALID); one that is merely not tight costs nothing but the shortcut; one that
 * does not hold (a ciphertext with more terms than stated) is the caller's error, as wrong offsets would be. */
int csgn_decrypt_ragged_bounded(uint64_t n_bits, uint64_t batch, uint64_t total_terms, uint64_t max_terms,
                                const uint64_t *d_terms, const uint64_t *d_off, const uint64_t *d_mask,
                                uint8_t *d_bits, void *d_scratch, void *stream);

/* Fused forms: the plaintext of a product / sum WITHOUT materialising it.
 *     bit_b = Dec(L_b * R_b) = Dec(L_b) & Dec(R_b)        (product)
 *     bit_b = Dec(L_b + R_b) = Dec(L_b) ^ Dec(R_b)        (sum)
 * exact identities of the scheme: a product term L_i & R_j has all D secret positions set
 * iff both factors do, so the count of such terms is hits(L)*hits(R); concatenation adds the
 * counts (src/SecretKey.cpp:131-140 applied to src/Ciphertext.cpp:153-163 / :107-122).
 * Reads 8*dL*(t1+t2) bytes per pair instead of writing 8*dL*t1*t2.  d_scratch must hold
 * csgn_decrypt_combined_scratch_bytes(batch, t1, t2) bytes. */
size_t csgn_decrypt_combined_scratch_bytes(uint64_t batch, uint64_t t1, uint64_t t2);
int csgn_decrypt_product_uniform(uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2,
                                 const uint64_t *d_left, const uint64_t *d_right,
                                 const uint64_t *d_mask, uint8_t *d_bits, void *d_scratch, void *stream);
int csgn_decrypt_sum_uniform(uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2,
                             const uint64_t *d_left, const uint64_t *d_right,
                             const uint64_t *d_mask, uint8_t *d_bits, void *d_scratch, void *stream);

/* EXTENSION, not reference behaviour: mod-2 compaction of term lists.  The
 * reference's add never reduces (src/Ciphertext.cpp:107-122); because decryption XORs over
 * terms (src/SecretKey.cpp:139), identical terms cancel in pairs, so every ciphertext may be
 * replaced by its distinct odd-multiplicity terms without changing Dec under ANY key.  Output
 * keeps one copy of each such term at the position order of first occurrence; d_off_out
 * receives the compacted CSR offsets (d_off_out[batch] = terms kept).  d_out needs room for
 * total_terms*dL words and must not overlap d_terms; d_scratch needs
 * csgn_compact_scratch_bytes(n_bits, batch, total_terms) bytes.
 * max_terms: an upper bound on the term count of any ONE ciphertext of the batch when the caller
 * knows it, 0 = unknown.  It is a launch hint only: a ciphertext up to one workgroup's group (1024
 * terms at N=1247, 320 at N=4096) is read once and deduplicated in LDS; with a bound of up to 1792 / 768
 * terms a wide build of the same kernel (48 units per lane, one workgroup per CU) does the same for the
 * whole batch; larger ciphertexts are deduplicated by hash partitions (terms read twice; an exact table
 * in HBM behind a partition overflow or a hash collision) whose kernels are skipped when the bound rules
 * them out; a bound under half a group lets runs of small ciphertexts fill their groups.  A ciphertext
 * that exceeds a non-zero group-sized bound it was promised to respect is copied through uncompacted
 * (still a legal result); a broken small bound sends the call back to the plan it would have had without one.
 * Bit-exact for every input: terms are matched by a hash (48-bit tags inside a group, 64 bits between the
 * chunks of a larger ciphertext) first and then compared in full; a collision between unequal terms only
 * costs time.
 * Limits: fewer than 2^31 ciphertexts and terms per call (CSGN_ERR_UNSUPPORTED).
 * Never called on a parity path. */
size_t csgn_compact_scratch_bytes(uint64_t n_bits, uint64_t batch, uint64_t total_terms);
int csgn_compact_ragged(uint64_t n_bits, uint64_t batch, uint64_t total_terms, uint64_t max_terms,
                        const uint64_t *d_terms, const uint64_t *d_off,
                        uint64_t *d_out, uint64_t *d_off_out, void *d_scratch, void *stream);

/* ------------------------------------------------------------------- encrypt ---- */

/* Batched SecretKey::encrypt (bit vector src/SecretKey.cpp:35-80, MSB-first packing
 * :153-206) with the randomness made an explicit argument (hard part 3).
 * For ciphertext b:
 *   d_rnd[b*dL ..]  the value rand()%2 the reference would have stored at each position,
 *                   packed MSB-first (forced positions are ignored);
 *   d_chosen[b]     for plaintext 0: the secret POSITION s[rand()%d] picked at :51;
 *   d_last[b]       for plaintext 0: the final rand()%2 of :76 (used only when the other
 *                   secret positions are not all 1).
 * bit 1: out = rnd | mask.   bit 0: out = rnd with position `chosen` replaced by
 * (all other secret positions are 1) ? 0 : last -- for D==1 the reference never clears it
 * (its `v` stays 0), and neither does this.  Padding bits of the last word are cleared.
 * The certFHE::SecretKey class maps the glibc rand() stream onto these arrays, which makes
 * the device result bit-identical to the reference under the same srand(). */
int csgn_encrypt_explicit(uint64_t n_bits, uint64_t d, uint64_t batch,
                          const uint8_t *d_plain, const uint64_t *d_rnd,
                          const uint32_t *d_chosen, const uint8_t *d_last,
                          const uint64_t *d_mask, uint64_t *d_out, void *stream);
/* Throughput form: same construction, randomness generated on the device by a KEYED generator:
 * ChaCha (64-bit block counter, 64-bit nonce; 8, 12 or 20 rounds) in counter mode under a 256-bit
 * secret key.  Outputs do not reveal the key or one another (a ciphertext word that carries no
 * secret position IS raw generator output, so an invertible generator would leak the stream and
 * with it the secret positions).  Same distribution as the reference, not the same bits: every
 * position is drawn; plaintext 1 ORs the key mask in; for plaintext 0, if all D secret positions
 * came out 1, position s[draw % D] is cleared (equivalent to src/SecretKey.cpp:51-76: draw the
 * position first, force it to 0 when all the others are 1) -- unless the key has a single distinct
 * position, which the reference never clears either.  `draw` comes from a second stream of the same
 * (key, nonce) whose ChaCha constants are "csgn draw pos v1" instead of "expand 32-byte k": no nonce
 * makes it coincide with a keystream.
 *   h_rng              key/nonce/rounds (host struct; fill with csgn_rng_from_os for real use)
 *   first_ciphertext   GLOBAL index of d_plain[0] / d_out[0] in the (key, nonce) stream: ciphertext
 *                      c always draws the same words whatever batch or shard it is encrypted in
 *                      (csgn_shard.h).  Never encrypt two different plaintexts under the same
 *                      (key, nonce, index): advance first_ciphertext or change the nonce.
 *   d_key              the D secret indices (device), d_mask their dL-word mask (csgn_key_mask).
 * Keystream layout (csgn_encrypt_keyed_layout reports U, P, Gc): U = ceil(dL/2) 16-byte units per
 * ciphertext, P = U/gcd(U,256), Gc = 256*P/U; unit j of ciphertext c is words 4q..4q+3 of ChaCha
 * block (g*P + p)*64 + L with g = c/Gc, r = (c%Gc)*U + j, p = r/256, q = (r%256)/64, L = r%64. */
typedef struct csgn_rng {
    uint32_t key[8];      /* 256-bit generator key: SECRET */
    uint64_t nonce;       /* stream id */
    uint32_t rounds;      /* 8, 12 or 20 */
    uint32_t reserved;
} csgn_rng;
/* key and nonce from the operating system's entropy source (getrandom). */
int csgn_rng_from_os(csgn_rng *h_rng, uint32_t rounds);
/* REPRODUCIBLE stream for tests and benchmarks: key and nonce expanded from a 64-bit seed.  Sixty-four
 * bits of entropy at most -- not for ciphertexts that have to stay secret. */
int csgn_rng_from_seed(csgn_rng *h_rng, uint64_t seed, uint32_t rounds);
int csgn_encrypt_keyed_layout(uint64_t n_bits, uint32_t *h_units, uint32_t *h_passes, uint32_t *h_group);
int csgn_encrypt_keyed(uint64_t n_bits, uint64_t d, uint64_t batch, uint64_t first_ciphertext,
                       const uint8_t *d_plain, const uint64_t *d_key, const uint64_t *d_mask,
                       const csgn_rng *h_rng, uint64_t *d_out, void *stream);
/* FUSED FRESH CHAIN (the reference's canonical flow tests/basic_operations.cpp:26-40:
 * encrypt, encrypt, operator*, decrypt).  For every pair b < batch
 *     d_out_b = Enc_A(d_plain_a[b]) & Enc_B(d_plain_b[b])          one term, dL words
 * where Enc_A / Enc_B are EXACTLY the ciphertexts csgn_encrypt_keyed(..., h_rng_a / h_rng_b, ...)
 * writes for position first_ciphertext + b and & is Ciphertext::defaultN_multiply
 * (src/Ciphertext.cpp:124-131).  One kernel: both operands live in registers only and the product is
 * written once -- 8*dL bytes per pair instead of the five HBM passes of encrypt, encrypt, multiply.
 * d_bits (optional, may be NULL) receives Dec(d_out_b) under the same key, one byte per pair, computed
 * from the generated words (a 1x1 product decrypts to 1 iff both factors cover the key mask,
 * src/SecretKey.cpp:82-102).  The two generators must differ in key or nonce. */
int csgn_encrypt_mul_keyed(uint64_t n_bits, uint64_t d, uint64_t batch, uint64_t first_ciphertext,
                           const uint8_t *d_plain_a, const uint8_t *d_plain_b, const uint64_t *d_key,
                           const uint64_t *d_mask, const csgn_rng *h_rng_a, const csgn_rng *h_rng_b,
                           uint64_t *d_out, uint8_t *d_bits, void *stream);
/* = csgn_encrypt_keyed with csgn_rng_from_seed(seed, 8 rounds) and first_ciphertext 0: the
 * reproducible test/benchmark form (see csgn_rng_from_seed: NOT for secrets). */
int csgn_encrypt_device_rng(uint64_t n_bits, uint64_t d, uint64_t batch,
                            const uint8_t *d_plain, const uint64_t *d_key,
                            const uint64_t *d_mask, uint64_t seed, uint64_t *d_out, void *stream);

/* --------------------------------------------------------------- permutation ---- */

/* Batched Ciphertext::applyPermutation (src/Ciphertext.cpp:7-82): new bit j = old bit
 * perm[j].  d_perm: N uint32 indices.  The reference collapses a multi-term ciphertext to
 * its permuted FIRST term; `per_term` = 0 reproduces that (d_out: batch*dL
 * words, input stride terms_in*dL), `per_term` = 1 permutes every term (extension,
 * d_out: batch*terms_in*dL). */
int csgn_permute_uniform(uint64_t n_bits, uint64_t batch, uint64_t terms_in, int per_term,
                         const uint64_t *d_terms, const uint32_t *d_perm, uint64_t *d_out,
                         void *stream);

/* ------------------------------------------- explicit bitlen (one ciphertext) ---- */

/* A ciphertext built through the reference's 4-argument constructor / setBitlen may carry ANY
 * bitlen side array; the reference then reads (v, bitlen) as a bit stream -- word i contributes its
 * top bitlen[i] bits -- and addresses it at flat positions (src/SecretKey.cpp:104-147,
 * src/Ciphertext.cpp:16-69).  These two calls do exactly that for ONE ciphertext of len_words words,
 * with d_bitlen[len_words] on the device (values above 64 are read as 64; a position past the end of
 * the stream reads 0):
 *   decrypt:  *d_bit = XOR over k < len_words/dL of AND over i < d of stream[n*k + key[i]]
 *             (d_key: the D indices themselves, not the mask -- positions are stream positions);
 *   permute:  d_out[dL words]: new bit j = stream[perm[j]] for j < min(N, stream length), the rest 0
 *             (as in the reference the result is ONE term).
 * d_scratch: csgn_bitlen_scratch_bytes(len_words).  With the canonical pattern both agree with
 * csgn_decrypt_uniform / csgn_permute_uniform, which are the fast paths. */
size_t csgn_bitlen_scratch_bytes(uint64_t len_words);
int csgn_decrypt_bitlen(uint64_t n_bits, uint64_t d, uint64_t len_words, const uint64_t *d_v,
                        const uint64_t *d_bitlen, const uint64_t *d_key, uint8_t *d_bit, void *d_scratch,
                        void *stream);
int csgn_permute_bitlen(uint64_t n_bits, uint64_t len_words, const uint64_t *d_v, const uint64_t *d_bitlen,
                        const uint32_t *d_perm, uint64_t *d_out, void *d_scratch, void *stream);

/* ------------------------------------------------------------------- harness ---- */

/* Synthetic operand words: word idx = splitmix64(seed + GOLDEN*(idx+1)), the
 * last word of each term masked to its top N%64 bits (the test checker restates this
 * definition independently). */
int csgn_synth_fill(uint64_t seed, uint64_t n_bits, uint64_t first_word, uint64_t n_words,
                    uint64_t *d_out, void *stream);
/* 64-bit order-sensitive digest, ADDED into *d_digest (zero it first):
 * sum_i splitmix64(w[i] + GOLDEN*(first_index+i+1)). */
int csgn_digest(const uint64_t *d_words, uint64_t n_words, uint64_t first_index,
                uint64_t *d_digest, void *stream);

/* ------------------------------------------------------------------ circuits ---- */

/* A fixed circuit of adds, multiplies and decrypts over uniform batches of `batch` ciphertexts
 * (the "circuit runner" of SURVEY 8f-2): every value lives in one HBM block owned by the
 * circuit, and csgn_circuit_build captures all launches into a hipGraph, so a launch-bound
 * circuit (BASELINE config 5: 24 operations of a few microseconds each on single ciphertexts)
 * replays with one graph launch.  Values are numbered from 0 in creation order.  Usage:
 * create; input()*; add()/mul()/decrypt()*; build(); then, per evaluation, write the inputs to
 * csgn_circuit_value(c, id) (batch*terms*dL words each, e.g. csgn_memcpy_d2d or an encrypt
 * kernel writing there directly), csgn_circuit_run, and read results / csgn_circuit_bits after
 * synchronising the stream.  Results are the same words the one-by-one calls produce. */
typedef struct csgn_circuit csgn_circuit;
int csgn_circuit_create(uint64_t n_bits, uint64_t batch, csgn_circuit **circuit);
void csgn_circuit_destroy(csgn_circuit *circuit);
int csgn_circuit_input(csgn_circuit *circuit, uint64_t terms, uint32_t *value);
/* A RAGGED input: element i has h_terms[i] terms (batch entries on the host; 0 allowed).  Shapes are
 * static -- fixed when the circuit is described -- so every size downstream is known on the host, the
 * CSR offsets of every ragged value are uploaded once at build time and the graph needs no plan step.
 * add / mul with a ragged operand give a ragged result (the CSR kernels csgn_add_ragged /
 * csgn_mul_ragged); decrypt works on either kind; permute of a ragged value is not supported.  The
 * input's words go to csgn_circuit_value() in CSR order (element after element). */
int csgn_circuit_input_ragged(csgn_circuit *circuit, const uint64_t *h_terms, uint32_t *value);
int csgn_circuit_add(csgn_circuit *circuit, uint32_t a, uint32_t b, uint32_t *value);   /* a + b: concatenation */
int csgn_circuit_mul(csgn_circuit *circuit, uint32_t a, uint32_t b, uint32_t *value);   /* a * b: all-pairs AND */
/* Decrypt value `a` under the key whose dL-word mask is d_mask (must stay valid); *bits_id
 * names a `batch`-byte result buffer. */
int csgn_circuit_decrypt(csgn_circuit *circuit, uint32_t a, const uint64_t *d_mask, uint32_t *bits_id);
/* EXTENSION (as csgn_compact_ragged, never on a parity path): value = a with every element reduced to its
 * distinct terms of odd multiplicity -- the one node that bounds the growth of a long add/multiply chain.
 * Its sizes are data: the result (and everything computed from it) is a DYNAMIC ragged value -- the shapes the
 * circuit knows for it are upper bounds (they size buffers and launches: csgn_circuit_value_total_terms), the
 * real CSR offsets are written by the device in every run (csgn_circuit_value_offsets; element batch = the
 * real total).  add / mul / decrypt / compact accept dynamic values (mul through the kernels of
 * csgn_mul_ragged_async); permute does not. */
int csgn_circuit_compact(csgn_circuit *circuit, uint32_t a, uint32_t *value);
/* Ciphertext::applyPermutation on every element of value `a` (d_perm: N uint32 entries, must stay
 * valid): as in the reference the result is ONE term, the permuted first term. */
int csgn_circuit_permute(csgn_circuit *circuit, uint32_t a, const uint32_t *d_perm, uint32_t *value);
/* An INPUT produced inside the graph: batch fresh ciphertexts (one term each) of the plaintext bytes
 * at d_plain, encrypted by the keyed generator (csgn_encrypt_keyed) straight into the circuit's block:
 * no staging copy, and a fresh-ciphertext circuit Enc,Enc -> * / + -> Dec (BASELINE configs 2 and 4
 * end to end) replays as ONE graph launch.  d_plain (batch bytes), d_key (D indices) and d_mask stay
 * the caller's and must remain valid; rewrite d_plain between runs to encrypt other bits.  Element i
 * of run r (r = 1, 2, ...; csgn_circuit_epoch after csgn_circuit_run) draws stream position
 * first_ciphertext + i of the generator (node key, nonce = r), where the NODE KEY is derived here,
 * on the host, from (h_rng->key, h_rng->nonce) -- csgn_circuit_node_key -- and the nonce words carry
 * nothing but the run number: the graph's first node increments the run counter on the device, so no
 * replay re-uses a keystream, and no choice of nonce by the caller can make one node's run r the run
 * r' of another.  Give every encrypt node of a circuit its own first_ciphertext range (or its own
 * h_rng->nonce). */
int csgn_circuit_encrypt(csgn_circuit *circuit, uint64_t d, const uint8_t *d_plain, const uint64_t *d_key,
                         const uint64_t *d_mask, const csgn_rng *h_rng, uint64_t first_ciphertext,
                         uint32_t *value);
/* The fused fresh chain as ONE node (csgn_encrypt_mul_keyed inside the graph): value = Enc_A(d_plain_a) *
 * Enc_B(d_plain_b), one term per element, and -- when bits_id is not NULL -- its decryption under the same
 * key as a result buffer.  BASELINE configs 2 / 4 end to end (encrypt, encrypt, multiply, decrypt) are
 * then two graph nodes (run counter + this kernel) and one pass over 8*dL bytes per pair.  The operands
 * themselves are never materialised; a circuit that needs them as values uses csgn_circuit_encrypt and
 * csgn_circuit_mul instead (a tape circuit never rewrites what the caller described: every value it was asked
 * for stays addressable through csgn_circuit_value).  Keys, nonces and runs as for csgn_circuit_encrypt. */
int csgn_circuit_encrypt_mul(csgn_circuit *circuit, uint64_t d, const uint8_t *d_plain_a, const uint8_t *d_plain_b,
                             const uint64_t *d_key, const uint64_t *d_mask, const csgn_rng *h_rng_a,
                             const csgn_rng *h_rng_b, uint64_t first_ciphertext, uint32_t *value, uint32_t *bits_id);
uint64_t csgn_circuit_epoch(const csgn_circuit *circuit);      /* runs launched so far */
/* The key a circuit encrypt node built from *h_rng encrypts under: words 0..7 of the ChaCha20 block
 * (constants "csgn node key v1", key = h_rng->key, nonce = h_rng->nonce, counter 0).  Host only. */
int csgn_circuit_node_key(const csgn_rng *h_rng, uint32_t h_node_key[8]);
/* COMPILED circuits (round 5; SURVEY 8f-2 "never materialise").  By default a circuit is a TAPE: every value it was
 * asked for is written to a region of its own and stays addressable after every run, one kernel per node.
 * csgn_circuit_optimize(flags != 0) before csgn_circuit_build turns the build into a compiler: only inputs, the
 * values named by csgn_circuit_output and the decrypt bits survive a run (csgn_circuit_value returns NULL for
 * every other value), and the passes selected by `flags` arrange the rest:
 *   CSGN_CIRCUIT_REUSE         liveness -- the graph is a chain of kernel nodes, so the region of a value is handed
 *                              out again once its last reader has been emitted: the block is the peak live set
 *                              (csgn_circuit_block_bytes), not the sum of all values;
 *   CSGN_CIRCUIT_PLACE         add is concatenation (src/Ciphertext.cpp:107-122): a product or sum whose only
 *                              consumer is an add is written by its producer straight into its slice of the sum
 *                              (per-element output pitch) -- that operand's copy disappears; operands that cannot be
 *                              placed (inputs, shared values) are copied into their slice alone;
 *   CSGN_CIRCUIT_FUSE_DECRYPT  Dec(a*b) = Dec(a) & Dec(b), Dec(a+b) = Dec(a) ^ Dec(b) (src/SecretKey.cpp:131-140 XORs
 *                              hits over terms): a product or sum whose ONLY consumer is a decrypt is never computed,
 *                              its operands are decrypted and the bits combined -- ONE level;
 *   CSGN_CIRCUIT_PUSHDOWN      the same through every level of single-consumer values (a circuit that only asks for
 *                              bits then decrypts little more than its inputs); not part of CSGN_CIRCUIT_ALL;
 *   CSGN_CIRCUIT_HOIST         copies whose source is a circuit INPUT (an input added to a product, a sum of two
 *                              inputs) depend on nothing the graph computes: all of them go into ONE strided-copy
 *                              launch in front of the first node instead of a small launch each.
 * Nodes whose value nothing reads any more are dropped.  Shared sub-expressions are never fused or placed (a value
 * with two readers is materialised once).  Retained words and all bits are those of the tape, of the one-by-one
 * calls and of the reference.  The graph must be launched on the stream the inputs were written on, or after
 * synchronising with it. */
#define CSGN_CIRCUIT_REUSE 1u
#define CSGN_CIRCUIT_PLACE 2u
#define CSGN_CIRCUIT_FUSE_DECRYPT 4u
#define CSGN_CIRCUIT_PUSHDOWN 8u
#define CSGN_CIRCUIT_HOIST 16u
#define CSGN_CIRCUIT_ALL 23u
int csgn_circuit_optimize(csgn_circuit *circuit, uint32_t flags);
int csgn_circuit_output(csgn_circuit *circuit, uint32_t value);                /* keep this value materialised and addressable */
int csgn_circuit_build(csgn_circuit *circuit);
uint64_t csgn_circuit_block_bytes(const csgn_circuit *circuit);               /* size of the circuit's HBM block; 0 before build */
/* After build: {block bytes, algorithmic bytes of one run (reads + writes of every emitted kernel, SURVEY 8d's
 * per-operation figures), nodes described, kernels emitted, add operands placed (copies that disappeared),
 * decrypts fused, nodes dropped, input copies hoisted into the prologue launch}. */
int csgn_circuit_stats(const csgn_circuit *circuit, uint64_t h_stats[8]);
/* What csgn_circuit_build would do, without touching a device (host only, before build): a JSON object
 * {"bytes", "values": [{region, addressable, offset, pitch, parent, terms, total}], "ops": [{kind, a, b, out, elided,
 * placed_a, placed_b, expr}], "exprs": [{kind (-1 leaf, 0 xor, 1 and), value, l, r}], "regions": [{at, bytes, from, to}]}
 * -- `from`/`to` are the first node that writes and the last that reads a region (-1 = before the run, 2^31-1 = kept).
 * For tests of the compiler and for a caller who wants to see where the bytes of a circuit went. */
int csgn_circuit_plan_json(csgn_circuit *circuit, char *h_json, size_t cap);
uint64_t *csgn_circuit_value(csgn_circuit *circuit, uint32_t value);          /* device pointer; NULL before build, and for a value a compiled circuit did not retain */
uint64_t csgn_circuit_value_terms(csgn_circuit *circuit, uint32_t value);      /* per element; 0 for a ragged value */
uint64_t csgn_circuit_value_total_terms(csgn_circuit *circuit, uint32_t value); /* over the whole batch */
const uint64_t *csgn_circuit_value_offsets(csgn_circuit *circuit, uint32_t value);   /* device CSR offsets (batch+1) of a ragged value, NULL otherwise */
uint8_t *csgn_circuit_bits(csgn_circuit *circuit, uint32_t bits_id);          /* device pointer */
int csgn_circuit_run(csgn_circuit *circuit, void *stream);

/* Name of the kernel(s) a csgn_mul_uniform call of `pairs` pairs (its `batch` argument) of this
 * shape dispatches to ("k_and_stream", "k_mul_tiled", "k_mul_flat", "k_touch+k_mul_flat"); a
 * static string, no GPU needed.  Lets a profiler-driven harness (bench.py) label its roofline
 * with the kernel that really runs. */
const char *csgn_mul_uniform_kernel(uint64_t n_bits, uint64_t pairs, uint64_t t1, uint64_t t2);

/* ------------------------------------------------------------- gates ---- */

/* Plaintext constants and the boolean gates they make possible (uniform batches).  `+` (XOR) and `*` (AND) both map
 * 0 to 0, so without a constant every computable function maps the all-zero input to 0, and whoever evaluates holds no
 * key to encrypt a 1.  But a term decrypts to the AND of the key's d positions in it (src/SecretKey.cpp:82-147): the
 * ALL-ONES term (every word ~0, the last word masked to its top N%64 bits as in every canonical term) decrypts to 1 under
 * every key, the all-zero term to 0.  These are TRIVIAL encryptions: their plaintext is public, and an output that is
 * only a constant hides nothing.
 *
 * Every gate is a composition of the reference's operator+ / operator* (src/Ciphertext.cpp:107-179) in this order,
 * so its words are those of that composition (ONE / ZERO: one all-ones / all-zero term):
 *     NOT a        a + ONE                              ta + 1 terms            reads a
 *     XNOR(a,b)    (a + b) + ONE                        ta + tb + 1             reads a, b
 *     NAND(a,b)    (a * b) + ONE                        ta*tb + 1               reads a, b
 *     OR(a,b)      (a + b) + (a * b)                    ta + tb + ta*tb         reads a, b
 *     NOR(a,b)     ((a + b) + (a * b)) + ONE            ta + tb + ta*tb + 1     reads a, b
 *     MUX(s,a,b)   (s * (a + b)) + b     (s ? a : b)    ts*(ta + tb) + tb       reads sel, a, b
 *     ADD_PLAIN    a + (p ? ONE : ZERO)                 ta + 1                  reads a, plain
 *     MUL_PLAIN    a * (p ? ONE : ZERO)                 ta                      reads a, plain
 * p = d_plain[e] & 1, one public bit per element (ZERO keeps the batch uniform when p = 0). */
enum {
    CSGN_GATE_NOT = 1,
    CSGN_GATE_XNOR,
    CSGN_GATE_NAND,
    CSGN_GATE_OR,
    CSGN_GATE_NOR,
    CSGN_GATE_MUX,
    CSGN_GATE_ADD_PLAIN,
    CSGN_GATE_MUL_PLAIN
};
/* Terms per output element (host only).  0: unknown gate, a term count of 0 in an operand the gate reads, or overflow. */
uint64_t csgn_gate_terms(int gate, uint64_t t_sel, uint64_t t_a, uint64_t t_b);
/* Which form a csgn_gate_uniform call of this shape takes (host only, a static string): "k_gate_fused" (one kernel:
 * operands read once, every segment of the output written in one pass) or "pitched" (small products fused, larger ones
 * through the tuned csgn_mul_uniform / csgn_add_uniform launchers writing into the output's slices, plus the constant
 * fill; no intermediate buffer).  Knob "gate_fused" (-1 per shape, 0 / 1 forced) decides; the words are the same.
 * MUL_PLAIN, and MUX with t_sel > 1, are always fused.  "" for an invalid gate or shape. */
const char *csgn_gate_uniform_kernel(uint64_t n_bits, int gate, uint64_t batch,
                                     uint64_t t_sel, uint64_t t_a, uint64_t t_b);
/* One gate over `batch` elements: d_out = batch * csgn_gate_terms(...) * dL words, element after element.  Pointers
 * the gate does not read (table above) may be NULL and their term counts are ignored.  d_a and d_b (and d_sel) may
 * alias one another; d_out overlaps no input.  Limits: csgn_gate_terms(...) * dL < 2^31 words per element
 * (CSGN_ERR_UNSUPPORTED), batch * that < 2^60.  On the caller's stream, asynchronous.  No GPU: CSGN_ERR_NO_DEVICE,
 * no CPU fallback. */
int csgn_gate_uniform(uint64_t n_bits, int gate, uint64_t batch, uint64_t t_sel, uint64_t t_a, uint64_t t_b,
                      const uint64_t *d_sel, const uint64_t *d_a, const uint64_t *d_b, const uint8_t *d_plain,
                      uint64_t *d_out, void *stream);
/* A batch of `batch` 1-term constants into d_out (batch * dL words): element e is ONE if d_plain[e] & 1, else ZERO;
 * d_plain NULL: every element is ONE if bit != 0, else ZERO.  Written by a kernel (graph-safe).  No GPU:
 * CSGN_ERR_NO_DEVICE. */
int csgn_const_fill(uint64_t n_bits, uint64_t batch, const uint8_t *d_plain, int bit, uint64_t *d_out, void *stream);

/* ----------------------------------------------------------- integers ---- */

/* Bit-sliced encrypted unsigned integers: a w-bit value is w planes, plane j = bit j (least significant first), each a
 * uniform batch.  Whole operations (certfhe/UInt.h) are chains of the per-bit STEPS below, each a composition of the
 * reference's operator+ / operator* with ONE (the gates above), in this order; x is the running value (carry,
 * equality or less-than so far):
 *     ADD_HALF(a, b)       out0 s = a + b                        ta + tb
 *                          out1 c = a * b                        ta*tb
 *     ADD_FULL(x=c, a, b)  out0 s = (a + b) + c                  ta + tb + tx
 *                          out1 c' = (a * b) + ((a + b) * c)     ta*tb + (ta + tb)*tx
 *     EQ_STEP(x=e, a, b)   out0 e' = e * ((a + b) + ONE)         tx*(ta + tb + 1)
 *     LT_FIRST(a, b)       out0 l = (a + ONE) * b                (ta + 1)*tb
 *     LT_STEP(x=l, a, b)   out0 l' = ((a + b) * (b + l)) + l     (ta + tb)*(tb + tx) + tx
 * ADD_HALF and LT_FIRST do not read x (t_x and d_x are ignored). */
enum { CSGN_UINT_ADD_HALF = 1, CSGN_UINT_ADD_FULL, CSGN_UINT_EQ_STEP, CSGN_UINT_LT_FIRST, CSGN_UINT_LT_STEP };
/* Terms per element of one output of a step (host only).  0: unknown step or output (only the ADD steps have output 1),
 * a term count of 0 in an operand the step reads, or overflow. */
uint64_t csgn_uint_step_terms(int step, int output, uint64_t t_x, uint64_t t_a, uint64_t t_b);
/* Which form a csgn_uint_step call of this shape takes (host only, a static string): "k_uint_step" (one kernel: every
 * segment of both outputs in one pass, operands read once, ONE made in registers) or "pitched" (the tuned
 * csgn_mul_uniform / csgn_add_uniform launchers writing into the outputs' slices; no
 * intermediate buffer).  Knob "uint_fused" (-1 per shape, 0 / 1 forced) decides; the words are the same.  A step whose
 * product rows interleave -- a concatenated right operand under a left operand of more than one term (EQ_STEP with
 * t_x > 1, LT_STEP with t_a or t_b > 1) -- is always fused.  "" for an invalid step or shape. */
const char *csgn_uint_step_kernel(uint64_t n_bits, int step, uint64_t batch, uint64_t t_x, uint64_t t_a, uint64_t t_b);
/* One step over `batch` elements: d_out0 = batch * csgn_uint_step_terms(step, 0, ...) * dL words, d_out1 (the carry of
 * the ADD steps) likewise for output 1, element after element.  d_out1 may be NULL: the carry is then neither computed
 * nor read; the other steps ignore it.  d_a and d_b may alias each other; no output overlaps an input.  Limits: each
 * output below 2^31 words per element (CSGN_ERR_UNSUPPORTED), batch * that < 2^60.  On the caller's stream,
 * asynchronous.  No GPU: CSGN_ERR_NO_DEVICE, no CPU fallback. */
int csgn_uint_step(uint64_t n_bits, int step, uint64_t batch, const uint64_t *d_x, uint64_t t_x, const uint64_t *d_a,
                   uint64_t t_a, const uint64_t *d_b, uint64_t t_b, uint64_t *d_out0, uint64_t *d_out1, void *stream);

/* Comparison of a w-bit integer (planes a_0..a_{w-1}, least significant first) against one PUBLIC constant k < 2^w for
 * the whole batch; one encrypted bit per element.  A fixed composition of the reference's operator+ / operator* with
 * ONE and ZERO (csgn_const_fill), in this order; n_j = a_j + ONE (logicNot); the running value is always the LEFT
 * operand of a product:
 *     EQ   g_j = k_j ? a_j : n_j;  e = g_0;  e = e * g_j  for j = 1..w-1
 *     LT   k == 0: ZERO.  m = lowest set bit of k;  l = n_m;  for j = m+1..w-1:
 *              k_j = 1: l = (l * a_j) + n_j        k_j = 0: l = l * n_j
 *     GT   k == 2^w-1: ZERO.  m = lowest clear bit of k;  l = a_m;  for j = m+1..w-1:
 *              k_j = 1: l = l * a_j                k_j = 0: l = (l * n_j) + a_j
 *     NE = EQ + ONE,  LE = GT + ONE,  GE = LT + ONE
 * Fresh 1-term planes: EQ has 2^(zeros of k) terms, LT at most 2^w, GT at most 2^w - 1. */
enum { CSGN_UINT_PLAIN_EQ = 1, CSGN_UINT_PLAIN_NE, CSGN_UINT_PLAIN_LT, CSGN_UINT_PLAIN_LE, CSGN_UINT_PLAIN_GT,
       CSGN_UINT_PLAIN_GE };
/* Terms per element of the result (host only); h_terms[j] = terms per element of plane j.  0: unknown cmp, width
 * outside 1..64, k >= 2^width, a plane of 0 terms, or a count of 2^62 or more. */
uint64_t csgn_uint_plain_terms(int cmp, uint64_t width, uint64_t k, const uint64_t *h_terms);
/* Which form a csgn_uint_plain call of this shape takes (host only, a static string): "k_uint_plain" (one kernel writes
 * the whole comparison, planes read in place, ONE and ZERO made in registers) or "composed" (the tuned
 * csgn_mul_uniform / csgn_add_uniform / csgn_const_fill launchers level by level, the running value in a temporary
 * block the calling thread keeps, under csgn_uint_addk's rules for its composed form).  Knob "uint_plain_fused" (-1 per shape, 0 / 1 forced) decides; the words are the
 * same.  Per shape (the knob at -1; a forced 0 / 1 holds for every shape): composed for width 1 and the ZERO results,
 * fused otherwise.  "" for an invalid shape. */
const char *csgn_uint_plain_kernel(uint64_t n_bits, int cmp, uint64_t batch, uint64_t width, uint64_t k,
                                   const uint64_t *h_terms);
/* One comparison over `batch` elements: h_planes is a HOST array of `width` device pointers (plane j: batch *
 * h_terms[j] * dL words, element after element), d_out = batch * csgn_uint_plain_terms(...) * dL words.  Planes may
 * alias one another; d_out overlaps no plane.  Limits: the result below 2^31 words per element (CSGN_ERR_UNSUPPORTED),
 * batch * that < 2^60.  On the caller's stream, asynchronous; the fused form is graph-capturable.  No GPU:
 * CSGN_ERR_NO_DEVICE, no CPU fallback. */
int csgn_uint_plain(uint64_t n_bits, int cmp, uint64_t batch, uint64_t width, uint64_t k,
                    const uint64_t *const *h_planes, const uint64_t *h_terms, uint64_t *d_out, void *stream);

/* csgn_uint_addk: a + k mod 2^w, planes a_0 ... a_{w-1} least significant first, plane j uniform with t_j terms per
 * element, 1 <= w <= 64, k < 2^w public and the same for every element.  A fixed composition of the reference's
 * operator+ / operator* with ONE, in this order; n_j = a_j + ONE; the running carry c is always the LEFT operand of a
 * product:
 *     k == 0:            out_j = a_j for every j (a copy, the same terms in the same order); carry-out = ZERO (one term)
 *     m = lowest set bit of k
 *     j <  m:            out_j = a_j
 *     j == m:            out_m = a_m + ONE                       c = a_m
 *     j >  m, k_j = 0:   out_j = a_j + c                         c = c * a_j
 *     j >  m, k_j = 1:   out_j = (a_j + c) + ONE                 c = (c * n_j) + a_j
 *     carry-out (optional, plane index w) = the c left after j = w-1
 * Terms per element: T(c) after plane m is t_m; after a plane with k_j = 0 it is T(c) * t_j, with k_j = 1 it is
 * T(c) * (t_j + 1) + t_j; out_j has t_j + T(c_j) + k_j terms for j > m, T(c_j) the count of the carry INTO plane j.
 * With fresh planes T(c) never exceeds 2^(set bits of k from bit m up to bit j) - 1, and a + 1 has 2 terms in every
 * plane.  (In clear bits: c * (1 ^ a) ^ a = a | c, the carry of a column whose constant bit is 1; c * a where it is 0.)
 * Derived operations add no new words:
 *     a - k      = a + ((2^w - k) mod 2^w)
 *     ~a         = a_j + ONE on every plane                       (logicNot of Gates.h)
 *     k - a      = ~(a + (~k mod 2^w))                            every plane of that sum, then + ONE
 *     -a         = 0 - a = ~(a + (2^w - 1)) */
/* Terms per element of every output into h_out_terms (host only): width + 1 counts, the last the carry-out's, without
 * the ONE of negate_out.  Returns 1, or 0 for a width outside 1..64, k >= 2^width, a null pointer, a plane of 0 terms
 * or a count of 2^62 or more (h_out_terms is then not written). */
int csgn_uint_addk_terms(uint64_t width, uint64_t k, const uint64_t *h_terms, uint64_t *h_out_terms);
/* Which form a csgn_uint_addk call of this shape takes (host only, a static string): "k_uint_addk" (one kernel writes
 * every output plane and the carry-out, planes read in place, ONE and ZERO made in registers) or "composed" (the tuned
 * csgn_add_uniform / csgn_mul_uniform / csgn_const_fill launchers plane by plane with pitched writes, the running carry
 * in a block the library keeps per host thread and stream, up to 256 MiB, grown when a call needs more).  Knob "uint_addk_fused" (-1 per shape, 0 / 1 forced) decides;
 * the words are the same.  Per shape, by measurement: composed for a single output plane (width 1 without
 * the carry-out), where the chain terms walk 8 levels or more on average (a + 1 from 16 bits up), for outputs of 16 GiB
 * or more with over 5 levels walked per term written, and where one element's planes pass a launch's 2^32 lanes; fused
 * otherwise.  "" for an invalid shape. */
const char *csgn_uint_addk_kernel(uint64_t n_bits, uint64_t batch, uint64_t width, uint64_t k, const uint64_t *h_terms,
                                  int with_carry);
/* The sum over `batch` elements: h_planes is a HOST array of `width` device pointers (plane j: batch * h_terms[j] * dL
 * words, element after element), h_outs a HOST array of `width` device pointers (output j: batch * (T_j + (negate_out ?
 * 1 : 0)) * dL words, T_j from csgn_uint_addk_terms), d_carry the carry-out (batch * T_width * dL words) or NULL: it is
 * then not computed.  negate_out != 0 appends ONE to every output plane (that is k' - a for the caller who passed
 * ~k'); the carry-out is never negated.  Inputs may alias one another; no output overlaps an input or another output.
 * Limits: every output below 2^31 words per element (CSGN_ERR_UNSUPPORTED), batch * that < 2^60.  On the caller's
 * stream, asynchronous; the fused form is one launch and graph-capturable.  The composed form is asynchronous once its
 * thread's block for that stream is large enough; a call that has to allocate or grow it calls hipMalloc (refused with
 * CSGN_ERR_HIP while the stream is capturing), and a temporary past 256 MiB is allocated for the call and freed behind
 * it, which waits for the device.  A thread keeps blocks for 8 streams per composed form; a ninth stream evicts the one
 * used least recently.  A call whose block is large enough can be captured into a graph; that block is then kept until
 * the thread ends, whatever grows or is evicted ("Graphs" at the top).  No GPU: CSGN_ERR_NO_DEVICE, no CPU fallback. */
int csgn_uint_addk(uint64_t n_bits, uint64_t batch, uint64_t width, uint64_t k, int negate_out,
                   const uint64_t *const *h_planes, const uint64_t *h_terms, uint64_t *const *h_outs, uint64_t *d_carry,
                   void *stream);

/* A PUBLIC lookup table f applied to a w-bit integer (planes a_0..a_{w-1}, least significant first, plane i uniform with
 * t_i terms per element): out_width output planes, output j encrypting bit j of f(x).  in_width 1..16, out_width 1..64,
 * h_table: 2^in_width entries, each < 2^out_width.  The words are the table's algebraic normal form over the planes, a
 * fixed composition of the reference's operator* / operator+ with ONE and ZERO (csgn_const_fill):
 *     anf = the Mobius transform of the table, bitwise on the whole word: for each i, for each x with bit i set,
 *           anf[x] ^= anf[x ^ (1 << i)];  bit j of anf[S] is the coefficient of the monomial S in output j
 *     M_S = ((a_{i1} * a_{i2}) * ...) over i in S ascending;  M_{} = ONE
 *     out_j = ((M_{S1} + M_{S2}) + ...) over the S with bit j of anf[S] set, ascending;  none: ZERO (one term)
 * Terms of output j: T_j = sum over those S of prod_{i in S} t_i (the empty S counts 1); 1 when the ANF is empty.
 * Fresh 1-term planes: T_j = |ANF(f_j)| <= 2^w. */
typedef struct csgn_uint_lut csgn_uint_lut;
/* Host only: the Mobius transform of the table into h_anf (2^in_width words).  CSGN_ERR_INVALID: a width outside its
 * range, a null pointer or an entry >= 2^out_width. */
int csgn_uint_lut_anf(uint64_t in_width, uint64_t out_width, const uint64_t *h_table, uint64_t *h_anf);
/* Host only: T_j of every output into h_out_terms (out_width words), for planes of h_terms[i] terms per element.
 * CSGN_ERR_INVALID for a bad argument, an entry >= 2^out_width, a plane of 0 terms or a count of 2^62 or more. */
int csgn_uint_lut_terms(uint64_t in_width, uint64_t out_width, const uint64_t *h_table, const uint64_t *h_terms,
                        uint64_t *h_out_terms);
/* Compiles the table for planes of h_terms[i] terms: the ANF, every output's monomial masks and their term offsets,
 * uploaded once (synchronous).  CSGN_ERR_UNSUPPORTED when an output reaches 2^31 terms; no GPU: CSGN_ERR_NO_DEVICE.
 * A compiled table is read-only: one may be applied from several host threads at once. */
int csgn_uint_lut_create(uint64_t in_width, uint64_t out_width, const uint64_t *h_table, const uint64_t *h_terms,
                         csgn_uint_lut **lut);
void csgn_uint_lut_destroy(csgn_uint_lut *lut);
/* Which form a csgn_uint_lut_apply call takes (host only, a static string): "k_uint_lut" (one kernel writes every
 * output plane, planes read in place, ONE and ZERO made in registers) or "composed" (csgn_mul_uniform /
 * csgn_add_uniform / csgn_const_fill monomial by monomial into the outputs' slices, partial products in a temporary
 * block the calling thread keeps, under csgn_uint_addk's rules for its composed form).  Knob "uint_lut_fused" (-1 per shape, 0 / 1 forced) decides; the words are the
 * same.  Per shape: fused.  "" for a null table or n_bits of 0. */
const char *csgn_uint_lut_kernel(uint64_t n_bits, const csgn_uint_lut *lut, uint64_t batch);
/* Applies the table over `batch` elements: h_planes is a HOST array of in_width device pointers (plane i: batch * t_i
 * * dL words), h_out a HOST array of out_width device pointers (output j: batch * T_j * dL words).  Planes may alias one
 * another; no output overlaps a plane or another output.  Limits: every T_j * dL below 2^31 words per element
 * (CSGN_ERR_UNSUPPORTED), batch * that < 2^60.  On the caller's stream, asynchronous; the fused form is one launch and
 * graph-capturable.  No GPU: CSGN_ERR_NO_DEVICE, no CPU fallback. */
int csgn_uint_lut_apply(const csgn_uint_lut *lut, uint64_t n_bits, uint64_t batch, const uint64_t *const *h_planes,
                        uint64_t *const *h_out, void *stream);

/* ------------------------------------------------------ gather / tile / broadcast ---- */

/* Data movement between batches: output element e is a bit-for-bit copy of source element idx[e] -- the same terms in
 * the same order, so the same words.  Indices are uint64 device words in any order and may repeat; count_out may be 0,
 * smaller than count_in or larger.  Both counts stay below 2^32.  d_index == NULL selects the TILE form,
 * idx[e] = e mod count_in; with count_in == 1 that is a BROADCAST.  Shapes: a uniform source of t terms per element
 * gives a uniform output of t terms per element; a ragged (CSR) source gives a ragged output whose offsets are the
 * exclusive prefix sums of the gathered elements' term counts (an element of 0 terms stays at 0 terms).  An index
 * >= count_in is an error: csgn_gather_plan reports it, and no kernel reads outside the source or its offsets because
 * of one.  A nonempty output needs count_in >= 1 (CSGN_ERR_INVALID otherwise).  No GPU: CSGN_ERR_NO_DEVICE, no CPU
 * fallback. */
/* Validates the index list and, for a ragged source (d_src_off != NULL, count_in + 1 words), writes the output offsets
 * to d_out_off (count_out + 1 words) and sets h_result[0] to the output's total terms.  Uniform source
 * (d_src_off == NULL): validation only, h_result[0] = 0.  h_result[1] = the number of indices >= count_in; when it is
 * nonzero the call returns CSGN_ERR_INVALID and d_out_off is not written.  Runs on the device (the prefix sum never
 * leaves it) and is SYNCHRONOUS: it hands sizes to the host.  d_index == NULL: the tile form (nothing to validate). */
int csgn_gather_plan(uint64_t count_in, const uint64_t *d_src_off, uint64_t count_out, const uint64_t *d_index,
                     uint64_t *d_out_off, uint64_t *h_result, void *stream);
/* The gather itself, one launch per 2^32 workgroups' worth of output (in practice one), asynchronous on the caller's
 * stream and graph-capturable.  Uniform source: d_src_off and d_dst_off NULL, t_src terms per element (t_src * dL
 * below 2^31 words), d_dst: count_out * t_src * dL words.  Ragged source: d_src_off (count_in + 1 words), d_dst_off
 * from csgn_gather_plan of the same index list, total_terms_out = its h_result[0], d_dst: total_terms_out * dL words;
 * t_src is ignored.  The index list must have passed a plan: the kernel still compares every index with count_in
 * before it follows it and leaves an element whose index fails unwritten.  Outputs below 2^60 words. */
int csgn_gather(uint64_t n_bits, uint64_t count_in, const uint64_t *d_src, const uint64_t *d_src_off, uint64_t t_src,
                uint64_t count_out, const uint64_t *d_index, uint64_t *d_dst, const uint64_t *d_dst_off,
                uint64_t total_terms_out, void *stream);
/* The UIntBatch form: n_planes (1..64) UNIFORM planes of count_in elements, plane j of h_terms[j] terms per element
 * (0: an empty plane, nothing written), gathered by ONE index list (or the tile form) into h_dst[j]
 * (count_out * h_terms[j] * dL words) in ONE launch.  h_src / h_dst / h_terms are HOST arrays of n_planes entries. */
int csgn_gather_planes(uint64_t n_bits, uint64_t n_planes, const uint64_t *const *h_src, const uint64_t *h_terms,
                       uint64_t count_in, uint64_t count_out, const uint64_t *d_index, uint64_t *const *h_dst,
                       void *stream);
/* Host only, a static string: the kernel a csgn_gather / csgn_gather_planes call launches -- "k_gather" (uniform
 * planes, indexed or tile), "k_gather_ragged" (a ragged source; n_planes must be 1), "none" (count_out == 0), ""
 * (n_bits == 0, n_planes outside 1..64, or a ragged plane table). */
const char *csgn_gather_kernel(uint64_t n_bits, uint64_t count_out, int ragged, uint64_t n_planes);

/* ------------------------------------------- encrypted tables at encrypted indices ---- */

/* An ENCRYPTED table read at an ENCRYPTED index.  Index: index_width = v planes x_0..x_{v-1} (bit 0 first, v in 1..16)
 * of `batch` elements, plane k uniform with s_k terms per element.  Table: `width` planes d_0..d_{width-1} (1..64) of
 * `rows` elements (1 <= rows <= 2^v), plane j uniform with t_j terms per element.  Output: `width` planes of `batch`
 * elements.  A fixed composition of the reference's operator+ / operator* with ONE:
 *     out_j = ((EQ(x, 0) * d_{0,j}) + (EQ(x, 1) * d_{1,j})) + ... + (EQ(x, rows-1) * d_{rows-1,j})   (left-nested)
 *     EQ(x, r)   the EQ row of csgn_uint_plain with k = r over element e's planes:  g_k = r_k ? x_k : (x_k + ONE),
 *                EQ = ((g_0 * g_1) * ...) * g_{v-1}
 *     d_{r,j}    plane j of table element r, the same for every e;  EQ is the LEFT operand of every product
 * Decrypts to table[x] when x < rows, and to 0 in every plane when x >= rows.
 * Terms of output j: T_j = t_j * E,  E = sum over r < rows of prod_k R_k(r),  R_k(r) = r_k ? s_k : s_k + 1;
 * rows = 2^v: E = prod_k (2 s_k + 1).  Fresh 1-term index planes: E = 3^v (6561 at v = 8: about 1 MB per output plane
 * and element at N=1247) -- the scheme's own growth, as for csgn_uint_step's comparisons.
 * Term order (decoding needs no table): row r's terms form a block of t_j * prod_k R_k(r) terms, blocks ascending in r;
 * inside a block term (q, c) is at q * t_j + c, c the table term (fastest), and q's mixed-radix digits d_k < R_k run
 * with k = 0 slowest; d_k selects term d_k of x_k, and d_k = s_k (only for r_k = 0) selects ONE. */
/* E (host only); 0 for index_width outside 1..16, rows outside 1..2^index_width, a null pointer, an index plane of 0
 * terms or a count of 2^62 or more. */
uint64_t csgn_uint_read_terms(uint64_t index_width, const uint64_t *h_index_terms, uint64_t rows);
/* Which form a csgn_uint_read call of this shape takes (host only, a static string): "k_uint_read" (one kernel writes
 * every output plane, planes read in place, ONE made in registers) or "composed" (per row r: csgn_uint_plain's EQ into
 * a temporary the calling thread keeps (csgn_uint_addk's rules for its composed form), the broadcast of row r by csgn_gather_planes' tile form, csgn_mul_uniform into r's slice
 * of every output).  Knob "uint_read_fused" (-1 per shape, 0 / 1 forced) decides; the words are the same.  Per shape:
 * fused.  "" for an invalid shape (n_bits 0, a bad width, rows or term count). */
const char *csgn_uint_read_kernel(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *h_index_terms,
                                  uint64_t rows, uint64_t width, const uint64_t *h_table_terms);
/* The read over `batch` elements.  h_index: a HOST array of index_width device pointers (plane k: batch * s_k * dL
 * words), h_table: a HOST array of `width` device pointers (plane j: rows * t_j * dL words), h_out: a HOST array of
 * `width` device pointers (output j: batch * T_j * dL words).  Planes may alias one another; no output overlaps an input
 * or another output.  Limits: every T_j * dL below 2^31 words per element (CSGN_ERR_UNSUPPORTED), batch * that < 2^60.
 * On the caller's stream, asynchronous; the fused form is one launch and graph-capturable.  No GPU:
 * CSGN_ERR_NO_DEVICE, no CPU fallback. */
int csgn_uint_read(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *const *h_index,
                   const uint64_t *h_index_terms, uint64_t rows, uint64_t width, const uint64_t *const *h_table,
                   const uint64_t *h_table_terms, uint64_t *const *h_out, void *stream);

/* ------------------------------------------------ encrypted tables by encrypted key ---- */

/* An ENCRYPTED table looked up by an ENCRYPTED key: a private key-value lookup, a join, an associative memory.
 * Keys: key_width = v planes y_0..y_{v-1} (v in 1..16) of `rows` elements, plane k uniform with u_k terms per element.
 * Query: v planes x_0..x_{v-1} of `batch` elements, plane k uniform with s_k terms.  Values: `width` planes
 * d_0..d_{width-1} (0..64) of `rows` elements, plane j uniform with t_j terms.  rows >= 1, with no upper bound other
 * than the size limits below.  Output: `width` planes of `batch` elements and, optionally, the bit `member`.  A fixed
 * composition of the reference's operator+ / operator* with ONE; y_{r,k} and d_{r,j} are row r broadcast to every
 * query element:
 *     EQ(y_r, x)  equalTo(key row r, query) of certfhe/UInt.h, the key as a, the query as b:
 *                 g_k = (y_{r,k} + x_k) + ONE (logicXnor);  EQ = ((g_0 * g_1) * ...) * g_{v-1}  (the EQ_STEP chain:
 *                 the running value is the LEFT operand)
 *     out_j  = ((EQ(y_0, x) * d_{0,j}) + (EQ(y_1, x) * d_{1,j})) + ... + (EQ(y_{rows-1}, x) * d_{rows-1,j})   (left-nested)
 *     member =  (EQ(y_0, x) + EQ(y_1, x)) + ... + EQ(y_{rows-1}, x)
 * out_j decrypts to the XOR, over the rows whose key equals the query, of bit j of the row's value: with distinct keys
 * the matching row's value, or 0 when no key matches.  member decrypts to the parity of the number of matching rows:
 * with distinct keys, membership.
 * Terms: every row has the same P = prod_k (u_k + s_k + 1) EQ terms;  T_j = rows * P * t_j,  T_member = rows * P.
 * Fresh 1-term planes: P = 3^v -- the scheme's own growth, as for csgn_uint_step's comparisons.
 * Term order (decoding needs no table): row r's terms form a block of P * t_j terms, blocks ascending in r; inside a
 * block term (q, c) is at q * t_j + c, c the value term (fastest), and q's mixed-radix digits d_k < u_k + s_k + 1 run
 * with k = 0 slowest; d_k < u_k selects term d_k of y_{r,k}, u_k <= d_k < u_k + s_k term d_k - u_k of x_k, and
 * d_k = u_k + s_k selects ONE.  member is the same stream without the value factor. */
/* P (host only); 0 for key_width outside 1..16, a null pointer, a plane of 0 terms or a count of 2^62 or more. */
uint64_t csgn_uint_find_terms(uint64_t key_width, const uint64_t *h_key_terms, const uint64_t *h_query_terms);
/* Which form a csgn_uint_find call of this shape takes (host only, a static string): "k_uint_find" (one kernel writes
 * every output plane and member, planes read in place, ONE made in registers) or "composed" (per row r: the broadcast
 * of row r of the key and value planes by csgn_gather_planes' tile form, the XNOR gate and the EQ_STEPs of
 * csgn_gate_uniform / csgn_uint_step into a temporary the calling thread keeps (csgn_uint_addk's rules for its composed
 * form), csgn_mul_uniform into r's slice of every output and a pitched copy into r's slice of member).  Knob
 * "uint_find_form" (-1 per shape, 0 composed, 1 fused) decides; the words are the same.  Per shape: fused (DESIGN
 * 4.19: no measured shape has the composed form ahead).  "" for an invalid shape (n_bits 0, a bad width, no rows, a bad
 * term count, or width 0 without member). */
const char *csgn_uint_find_kernel(uint64_t n_bits, uint64_t batch, uint64_t key_width, const uint64_t *h_key_terms,
                                  const uint64_t *h_query_terms, uint64_t rows, uint64_t width,
                                  const uint64_t *h_value_terms, int with_member);
/* The lookup over `batch` query elements.  h_query: a HOST array of key_width device pointers (plane k: batch * s_k *
 * dL words), h_keys: a HOST array of key_width device pointers (plane k: rows * u_k * dL words), h_values: a HOST array
 * of `width` device pointers (plane j: rows * t_j * dL words), h_out: a HOST array of `width` device pointers (output
 * j: batch * T_j * dL words), d_member: batch * T_member * dL words, or NULL: it is then not computed.  width == 0 is
 * allowed only with d_member (h_values, h_value_terms and h_out are then not read); otherwise CSGN_ERR_INVALID.
 * Inputs may alias one another; no output overlaps an input or another output.  Limits: every T_j * dL and
 * T_member * dL below 2^31 words per element (CSGN_ERR_UNSUPPORTED), batch * that < 2^60.  On the caller's stream,
 * asynchronous; the fused form is one launch and graph-capturable.  No GPU: CSGN_ERR_NO_DEVICE, no CPU fallback. */
int csgn_uint_find(uint64_t n_bits, uint64_t batch, uint64_t key_width, const uint64_t *const *h_query,
                   const uint64_t *h_query_terms, uint64_t rows, const uint64_t *const *h_keys,
                   const uint64_t *h_key_terms, uint64_t width, const uint64_t *const *h_values,
                   const uint64_t *h_value_terms, uint64_t *const *h_out, uint64_t *d_member, void *stream);

/* ------------------------------------------------ the first row whose encrypted mask bit is set ---- */

/* PRIORITY: of the `group` = g rows of an output element (g in 1..64), the value of the FIRST one whose ENCRYPTED mask
 * bit is set -- the LIMIT 1 / EXISTS of a private query, first-fit, a priority encoder, find-first-set.
 * Mask: bits m_0..m_{g-1} per element, row r uniform with s_r >= 1 terms.  Values, optionally: `width` planes
 * d_0..d_{width-1} (0..64), plane j uniform with t_j terms; row r of output element e is element e * g + r of the plane
 * (the grouped layout of csgn_count).  Labels, optionally: one PUBLIC 64-bit constant L_r per row.  A fixed composition
 * of the reference's operator+ / operator* with ONE:
 *     n_r    = m_r + ONE                                  (csgn_gate_uniform's NOT: m_r's terms, then ONE)
 *     F_0    = m_0;   F_r = (((n_0 * n_1) * ...) * n_{r-1}) * m_r      (left-nested, the running product the LEFT operand)
 *     out_j  = ((F_0 * d_{0,j}) + (F_1 * d_{1,j})) + ... + (F_{g-1} * d_{g-1,j})        (left-nested, F the LEFT operand)
 *     any    =  (F_0 + F_1) + ... + F_{g-1}
 *     lab_i  =  the left-nested sum, ascending in r, of F_r over the rows r with bit i of L_r set
 * Exactly one F_r decrypts to 1 when any mask bit is set, the first; none does otherwise.  out_j decrypts to bit j of
 * the first set row's value, any to the OR of the mask bits, lab_i to bit i of the first set row's label; all to 0 when
 * no mask bit is set.  With L_r = r the label planes are the index of the first set row, with L_r = 1 << r the one-hot
 * F_r themselves.
 * Terms: P_r = s_r * prod_{i<r} (s_i + 1);  the F stream has Q = sum_r P_r = prod_r (s_r + 1) - 1 entries;
 * T_j = Q * t_j,  T_any = Q,  T_lab_i = the sum of P_r over the rows with bit i of L_r set.  Fresh masks: P_r = 2^r,
 * Q = 2^g - 1.
 * Term order (decoding needs no table): row r's entries form a block of P_r entries, blocks ascending in r; entry `in`
 * of block r has mixed-radix digits with that of m_r (base s_r) fastest, then those of n_{r-1} .. n_0 (base s_i + 1),
 * n_0 slowest; a digit d < s_i selects term d of m_i, the digit s_i of an n_i selects ONE.  Term q * t_j + c of out_j is
 * (entry q of the stream) & (term c of d_{r(q),j}), c fastest; any is the bare stream; lab_i is the bare stream with the
 * blocks of the rows whose label lacks bit i left out. */
/* P_row for row < group, Q for row == group (host only); 0 for group outside 1..64, a null pointer, a row of 0 terms,
 * row > group or a count of 2^62 or more. */
uint64_t csgn_uint_first_terms(uint64_t group, const uint64_t *h_mask_terms, uint64_t row);
/* T_lab_bit (host only); 0 for the same refusals, for bit > 63 or when no label has the bit: such a plane does not
 * exist for the C ABI, as with csgn_count's 2^j > group. */
uint64_t csgn_uint_first_label_terms(uint64_t group, const uint64_t *h_mask_terms, const uint64_t *h_labels,
                                     uint64_t bit);
/* The selection over `batch` output elements.  h_mask: a HOST array of n_mask device pointers.  n_mask == 1, the
 * grouped layout: one batch of batch * group elements, row r of element e its element e * group + r; the g counts of
 * h_mask_terms must then be equal.  n_mask == group (>= 2), the plane layout: row r is a batch of `batch` elements of
 * its own s_r terms -- what an integer's planes hand over.  h_values: a HOST array of `width` device pointers (plane j:
 * batch * group * t_j * dL words, always grouped), h_out: `width` device pointers (output j: batch * T_j * dL words),
 * d_any: batch * Q * dL words, or NULL: not computed.  h_label_bits: n_labels (0..64) strictly ascending bit indices,
 * each naming a plane that exists; h_labels: the g constants, read only when n_labels > 0; h_label_out: n_labels device
 * pointers (plane i: batch * T_lab * dL words).  At least one of width, d_any and n_labels asks for something.  Inputs
 * may alias one another in any way; no output overlaps an input or another output.
 * Checks, the first that fails giving the status, all before any device call: n_bits; group, n_mask, width, n_labels
 * and nothing asked for; host pointers; term counts, label bits and the grouped layout's counts (CSGN_ERR_INVALID);
 * every output's T * dL below 2^31 words per element and batch * that < 2^60 (CSGN_ERR_UNSUPPORTED); null device
 * pointers (CSGN_ERR_INVALID; not read when batch == 0); the device (CSGN_ERR_NO_DEVICE, no CPU fallback).  batch == 0
 * succeeds.  On the caller's stream, asynchronous, no scratch, graph-capturable: ONE launch of k_uint_first, split by
 * elements only at knob "launch_blocks" and at the HIP grid limit. */
int csgn_uint_first(uint64_t n_bits, uint64_t batch, uint64_t group, const uint64_t *const *h_mask, uint64_t n_mask,
                    const uint64_t *h_mask_terms, uint64_t width, const uint64_t *const *h_values,
                    const uint64_t *h_value_terms, uint64_t *const *h_out, uint64_t *d_any, uint64_t n_labels,
                    const uint64_t *h_labels, const uint64_t *h_label_bits, uint64_t *const *h_label_out, void *stream);

/* ------------------------------------------------ the k-th row whose encrypted mask bit is set ---- */

/* SELECT: of the `group` = g rows of an output element (g in 1..64), the value of the (slot + 1)-th one whose ENCRYPTED
 * mask bit is set -- LIMIT k / OFFSET s of a private query, oblivious compaction of the matching rows to the front,
 * select_k on a bit vector -- and "at least slot + 1 of these bits are set": HAVING COUNT(*) >= k, k-of-n voting, a
 * Hamming-distance threshold.
 * Mask: bits m_0..m_{g-1} per element, EVERY row uniform with the same t >= 1 terms (as in csgn_count: the digit blocks
 * have one size).  Values, optionally: `width` planes d_0..d_{width-1} (0..64), plane j uniform with t_j terms; row r of
 * output element e is element e * g + r of the plane (the grouped layout of csgn_uint_first).  Labels, optionally: one
 * PUBLIC 64-bit constant L_r per row.  Slot s: public, 0-based, s < g.  Write [x] for "x is odd".  A fixed composition of
 * the reference's operator+ / operator*: for a row r >= s
 *     G_{r,s} = the left-nested sum, over d ascending in s..r with [C(d, s)],
 *               over the d-subsets i_1 < ... < i_d of {0..r-1} in lexicographic order (csgn_count's order),
 *               of ((((m_{i_1} * m_{i_2}) * ...) * m_{i_d}) * m_r)          (d = 0, which only s = 0 has: m_r alone)
 *     out_j   = ((G_{s,s} * d_{s,j}) + (G_{s+1,s} * d_{s+1,j})) + ... + (G_{g-1,s} * d_{g-1,j})     G the LEFT operand
 *     valid   =  (G_{s,s} + G_{s+1,s}) + ... + G_{g-1,s}
 *     lab_i   =  the left-nested sum, ascending in r >= s, of G_{r,s} over the rows with bit i of L_r set
 * "Exactly s of the r rows above are set" is a symmetric function, so its ANF is a sum of elementary symmetric
 * polynomials e_d, the ones with [C(d, s)]; G_{r,s} multiplies it by m_r.  Exactly one G_{r,s} decrypts to 1 when more
 * than s mask bits are set, and r is then the (s + 1)-th set row; none does otherwise.  out_j decrypts to bit j of that
 * row's value, valid to "at least s + 1 bits are set" (every monomial has a unique largest row, so valid is the minimal
 * ANF of that threshold), lab_i to bit i of that row's label; all to 0 when at most s bits are set.
 * Terms: P_{r,s} = sum over d in s..r with [C(d, s)] of C(r, d) * t^(d+1);  the G stream has Q_s = sum_r P_{r,s} = sum
 * over d of [C(d, s)] * C(g, d+1) * t^(d+1) entries;  T_j = Q_s * t_j,  T_valid = Q_s,  T_lab_i = the sum of P_{r,s} over
 * the rows r >= s with bit i of L_r set.  Fresh masks: Q_0 = 2^g - 1 (csgn_uint_first's terms as a multiset, in another
 * order), Q_{g-1} = 1; g = 8 gives 255, 127, 135, 71, 93, 29, 9, 1 for s = 0..7, and Q_62 = 65 at g = 64.
 * Term order (decoding needs no table): blocks ascending in r; inside block r segments ascending in d; inside a segment
 * the subsets by lexicographic rank; inside a subset the digits in base t, i_1's slowest and m_r's fastest.  Term
 * q * t_j + c of out_j is (entry q of the stream) & (term c of d_{r(q),j}), c fastest; valid is the bare stream; lab_i is
 * the bare stream with the blocks of the rows whose label lacks bit i left out. */
/* P_{row,slot} for row < group (0 for a row below the slot: it has no entries), Q_slot for row == group (host only); 0 for
 * group outside 1..64, slot >= group, t_mask of 0 or of 2^62 or more, row > group or a count of 2^62 or more: binomials
 * and powers saturate, they never wrap. */
uint64_t csgn_uint_nth_terms(uint64_t group, uint64_t t_mask, uint64_t slot, uint64_t row);
/* T_lab_bit (host only); 0 for the same refusals, for a null pointer, for bit > 63 or when no row >= slot has the bit:
 * such a plane does not exist for the C ABI, as with csgn_uint_first's. */
uint64_t csgn_uint_nth_label_terms(uint64_t group, uint64_t t_mask, uint64_t slot, const uint64_t *h_labels,
                                   uint64_t bit);
/* The selection of ONE slot over `batch` output elements (slots share no entries; a caller that wants slots 0..k-1 makes
 * k calls).  h_mask: a HOST array of n_mask device pointers.  n_mask == 1, the grouped layout: one batch of batch * group
 * elements, row r of element e its element e * group + r.  n_mask == group (>= 2), the plane layout: row r is a batch of
 * `batch` elements -- what an integer's planes hand over.  Either way every row has t_mask terms.  h_values: a HOST
 * array of `width` device pointers (plane j: batch * group * t_j * dL words, always grouped), h_out: `width` device
 * pointers (output j: batch * T_j * dL words), d_valid: batch * Q_slot * dL words, or NULL: not computed.  h_label_bits:
 * n_labels (0..64) strictly ascending bit indices, each naming a plane that exists; h_labels: the g constants, read only
 * when n_labels > 0; h_label_out: n_labels device pointers (plane i: batch * T_lab * dL words).  At least one of width,
 * d_valid and n_labels asks for something.  Inputs may alias one another in any way; no output overlaps an input or
 * another output.
 * Checks, the first that fails giving the status, all before any device call: n_bits; group, slot, n_mask, width,
 * n_labels and nothing asked for; host pointers; term counts (t_mask, Q_slot of 2^62 or more, the value planes') and
 * label bits (CSGN_ERR_INVALID); the stream's Q_slot * dL and every output's T * dL below 2^31 words per element and
 * batch * that < 2^60 (CSGN_ERR_UNSUPPORTED, no wrap-around; the stream is sized whatever is asked for, because the
 * kernel indexes it); null device pointers (CSGN_ERR_INVALID; not read when batch == 0); the device (CSGN_ERR_NO_DEVICE,
 * no CPU fallback).  batch == 0 succeeds.  On the caller's stream, asynchronous, no scratch, no plan object,
 * graph-capturable: ONE launch of k_uint_nth, split by elements only at knob "launch_blocks" and at the HIP grid limit. */
int csgn_uint_nth(uint64_t n_bits, uint64_t batch, uint64_t group, uint64_t slot, const uint64_t *const *h_mask,
                  uint64_t n_mask, uint64_t t_mask, uint64_t width, const uint64_t *const *h_values,
                  const uint64_t *h_value_terms, uint64_t *const *h_out, uint64_t *d_valid, uint64_t n_labels,
                  const uint64_t *h_labels, const uint64_t *h_label_bits, uint64_t *const *h_label_out, void *stream);

/* ------------------------------------------------ selection by an encrypted comparison ---- */

/* min, max and compare-exchange of ENCRYPTED integers: every output selected by the ENCRYPTED comparison a < b, the
 * step of every oblivious sort, top-k, median filter, arg-min and clamp.
 * Inputs: a and b, integers of `width` = w planes (w in 1..16, bit 0 first) of `batch` elements, plane j uniform with
 * ta_j / tb_j terms per element; n_out (0..64) requests, request i a pair of uniform planes (X_i, Y_i) of `batch`
 * elements with tx_i / ty_i terms; optionally the comparison itself.  A fixed composition of the reference's
 * operator+ / operator* with ONE:
 *     L      lessThan(a, b) of certfhe/UInt.h:  l_0 = (a_0 + ONE) * b_0,
 *            l_j = ((a_j + b_j) * (b_j + l_{j-1})) + l_{j-1}   (csgn_uint_step's LT_FIRST and LT_STEP rows),  L = l_{w-1}
 *     out_i  logicMux(L, X_i, Y_i) = (L * (X_i + Y_i)) + Y_i   (csgn_gate_uniform's MUX row, L the LEFT operand)
 * out_i decrypts to X_i where a < b and to Y_i elsewhere: a tie takes Y.  min is the requests (a_j, b_j), max the
 * requests (b_j, a_j), a payload that travels with the smaller key (pa_j, pb_j).
 * Terms: L_0 = (ta_0 + 1) * tb_0,  L_j = (ta_j + tb_j) * (tb_j + L_{j-1}) + L_{j-1};  T_i = L * (tx_i + ty_i) + ty_i
 * with L = L_{w-1}.  Fresh 1-term planes: L = 3^w - 1 -- the scheme's own growth, as for csgn_uint_step's comparisons.
 * Term order (decoding needs no table): term q * (tx_i + ty_i) + c of output i (q < L) is (term q of L) & (term c of
 * X_i when c < tx_i, else term c - tx_i of Y_i); the last ty_i terms are Y_i's, copied.  Term q of L, for j from w - 1
 * down to 1 with inner = tb_j + L_{j-1} and M = (ta_j + tb_j) * inner: q >= M lies in the tail copy (no factor of plane
 * j; go on with q - M); else p = q / inner names term p of a_j (p < ta_j) or term p - ta_j of b_j, and c = q % inner
 * term c of b_j (c < tb_j, which ends the walk) or entry c - tb_j of l_{j-1}.  At j = 0: p = q / tb_0 names term p of
 * a_0, or ONE when p = ta_0, ANDed with term q % tb_0 of b_0. */
/* L (host only); 0 for a width outside 1..16, a null pointer, a plane of 0 terms or a count of 2^62 or more. */
uint64_t csgn_uint_lt_terms(uint64_t width, const uint64_t *h_a_terms, const uint64_t *h_b_terms);
/* Which form a csgn_uint_lt_select call of this shape takes (host only, a static string): "k_uint_lt_select" (one kernel
 * writes every output and the comparison, planes read in place, the comparison never materialised) or "composed"
 * (LT_FIRST and the LT_STEPs through csgn_uint_step's launcher into a temporary the calling thread keeps
 * (csgn_uint_addk's rules for its composed form), csgn_gate_uniform's MUX launcher per output, a copy into d_less: what
 * select(lessThan(a, b), x, y) issues).  Knob "uint_lt_select_form" (-1 per shape, 0 composed, 1 fused) decides; the
 * words are the same.  Per shape: DESIGN 4.22.  "" for an invalid shape (n_bits 0, a bad width, more than 64 requests,
 * a bad term count, or no request without the comparison). */
const char *csgn_uint_lt_select_kernel(uint64_t n_bits, uint64_t batch, uint64_t width, const uint64_t *h_a_terms,
                                       const uint64_t *h_b_terms, uint64_t n_out, const uint64_t *h_x_terms,
                                       const uint64_t *h_y_terms, int with_less);
/* The selection over `batch` elements.  h_a, h_b: HOST arrays of `width` device pointers (plane j: batch * ta_j * dL and
 * batch * tb_j * dL words), h_x, h_y: HOST arrays of n_out device pointers (batch * tx_i * dL and batch * ty_i * dL
 * words), h_out: a HOST array of n_out device pointers (output i: batch * T_i * dL words), d_less: batch * L * dL words,
 * or NULL: the comparison is then not written.  n_out == 0 is allowed only with d_less (h_x, h_x_terms, h_y, h_y_terms
 * and h_out are then not read).  Inputs may alias one another, X_i = a_j included; no output overlaps an input or
 * another output.  Checks, in this order, the first that fails giving the status: n_bits; width; n_out; host pointers;
 * the term counts (CSGN_ERR_INVALID); L * dL and every T_i * dL below 2^31 words per element and batch times that below
 * 2^60 (CSGN_ERR_UNSUPPORTED; computed without wrap-around); null device pointers (CSGN_ERR_INVALID); the device
 * (CSGN_ERR_NO_DEVICE, no CPU fallback).  batch == 0 succeeds.  On the caller's stream, asynchronous; the fused form is
 * one launch for every shape within memory and graph-capturable. */
int csgn_uint_lt_select(uint64_t n_bits, uint64_t batch, uint64_t width, const uint64_t *const *h_a,
                        const uint64_t *h_a_terms, const uint64_t *const *h_b, const uint64_t *h_b_terms, uint64_t n_out,
                        const uint64_t *const *h_x, const uint64_t *h_x_terms, const uint64_t *const *h_y,
                        const uint64_t *h_y_terms, uint64_t *const *h_out, uint64_t *d_less, void *stream);

/* ------------------------------------------- sums, differences and equality of two integers ---- */

/* a + b, a - b, a == b and a != b of two ENCRYPTED integers, every plane of the result and the carry out of the top
 * plane in one launch: what certfhe/UInt.h's operator+, operator-, equalTo and notEqualTo compute.
 * Inputs: a and b, integers of `width` = w planes (w in 1..16, bit 0 first) of `batch` elements, plane j uniform with
 * ta_j / tb_j terms per element.  The words are those of the csgn_uint_step chains, term for term; a product of a left
 * term p and a right term q is term p * t_right + q:
 *     ADD  s_0, c_0 = ADD_HALF(a_0, b_0);  s_j, c_j = ADD_FULL(c_{j-1}, a_j, b_j);  the carry-out is c_{w-1}
 *     SUB  nb_j = b_j + ONE (csgn_gate_uniform's NOT), c_{-1} = ONE;  s_j, c_j = ADD_FULL(c_{j-1}, a_j, nb_j);
 *          a + ~b + 1: the carry-out c_{w-1} decrypts to 1 where a >= b
 *     EQ   e_0 = (a_0 + b_0) + ONE (the XNOR gate);  e_j = EQ_STEP(e_{j-1}, a_j, b_j);  the result is e_{w-1}
 *     NE   EQ + ONE
 * Terms: with tn_j = tb_j (SUB: tb_j + 1) and C_{-1} = 0 (SUB: 1), C_j = ta_j * tn_j + (ta_j + tn_j) * C_{j-1}; plane j
 * has ta_j + tn_j + C_{j-1} terms and the carry-out C_{w-1}.  EQ has prod_j (ta_j + tb_j + 1) terms, NE one more.  Fresh
 * 1-term planes: plane j of a sum has 2^j + 1 terms and its carry-out 2^w - 1; EQ has 3^w.
 * Term order (decoding needs no table): plane j is [a_j's terms | nb_j's terms | the entries of c_{j-1}], the ONE of
 * nb_j last (plane 0 of SUB ends in two ONEs: nothing cancels).  Entry q of c_j, for q < ta_j * tn_j, is term q / tn_j
 * of a_j ANDed with term q % tn_j of nb_j, which ends the walk; else, with q' = q - ta_j * tn_j, it is term
 * q' / C_{j-1} of the concatenation a_j | nb_j ANDed with entry q' % C_{j-1} of c_{j-1}.  Entry q of EQ is the
 * mixed-radix number whose fastest digit belongs to plane w - 1 and whose slowest to plane 0: digit d of plane j names
 * term d of a_j, term d - ta_j of b_j, or ONE (csgn_uint_find's decode of a key row against a query). */
enum { CSGN_UINT_ARITH_ADD = 1, CSGN_UINT_ARITH_SUB, CSGN_UINT_ARITH_EQ, CSGN_UINT_ARITH_NE };
/* Terms per element of one output (host only): output j < width is plane j of ADD / SUB and output `width` their
 * carry-out; output 0 is the result of EQ / NE.  0 for an unknown op, a width outside 1..16, a null pointer, a plane of
 * 0 terms, an output the op does not have, or a count of 2^62 or more. */
uint64_t csgn_uint_arith_terms(int op, uint64_t width, const uint64_t *h_a_terms, const uint64_t *h_b_terms,
                               uint64_t output);
/* Which form a csgn_uint_arith call of this shape takes (host only, a static string): "k_uint_arith" (one kernel writes
 * every plane and the carry, operands read in place, no running value materialised) or "composed" (the per-bit chain
 * above through csgn_uint_step's and csgn_gate_uniform's launchers, the running value in a temporary the calling thread
 * keeps (csgn_uint_addk's rules for its composed form)).  Knob "uint_arith_form" (-1 per shape, 0 the chain, 1 the one
 * launch) decides; the words are the same.  Per shape: DESIGN 4.28.  "" for an invalid shape (n_bits 0, an unknown op,
 * a bad width, a bad term count, or a carry asked of EQ / NE). */
const char *csgn_uint_arith_kernel(uint64_t n_bits, int op, uint64_t batch, uint64_t width, const uint64_t *h_a_terms,
                                   const uint64_t *h_b_terms, int with_carry);
/* The operation over `batch` elements.  h_a, h_b: HOST arrays of `width` device pointers (plane j: batch * ta_j * dL and
 * batch * tb_j * dL words), h_out: a HOST array of `width` device pointers for ADD / SUB (plane j: batch * T_j * dL
 * words) and of one for EQ / NE, d_carry: batch * C_{w-1} * dL words, or NULL: the carry is then neither computed nor
 * written; it must be NULL for EQ / NE.  Inputs may alias one another; no output overlaps an input or another output.
 * Checks, in this order, the first that fails giving the status: n_bits; op; width; host pointers (and a carry asked of
 * a comparison); the term counts (CSGN_ERR_INVALID); every output's T * dL below 2^31 words per element and batch
 * times that below 2^60 (CSGN_ERR_UNSUPPORTED; computed without wrap-around); null device pointers (CSGN_ERR_INVALID);
 * the device (CSGN_ERR_NO_DEVICE, no CPU fallback).  batch == 0 succeeds.  On the caller's stream, asynchronous; the
 * fused form is one launch for every shape within memory and graph-capturable. */
int csgn_uint_arith(uint64_t n_bits, int op, uint64_t batch, uint64_t width, const uint64_t *const *h_a,
                    const uint64_t *h_a_terms, const uint64_t *const *h_b, const uint64_t *h_b_terms,
                    uint64_t *const *h_out, uint64_t *d_carry, void *stream);

/* ------------------------------------- a public constant added where an encrypted flag is set ---- */

/* csgn_uint_add_where: a + (s ? k : 0) mod 2^w, every plane of the result and the carry out of the top plane in one
 * launch: what certfhe/UInt.h's addWhere, subWhere, incrementWhere and decrementWhere compute.  The inputs are:
 *   - a, an integer of w planes a_0 ... a_{w-1}, bit 0 first, plane j uniform with ta_j terms per element;
 *   - s, one uniform batch of ts terms per element, one encrypted bit per element;
 *   - k < 2^w, public and the same for every element.
 * The operation is a fixed composition of the reference's operator+ (concatenation) and operator* (all-pairs AND, the
 * left term slow).  It is the ADD chain of csgn_uint_step with b_j = s where k_j = 1 and b_j ABSENT where k_j = 0:
 *     k == 0:            out_j = a_j for every j (a copy: the same terms in the same order); carry-out = ZERO (one term)
 *     m = lowest set bit of k
 *     j <  m:            out_j = a_j
 *     j == m:            out_m = a_m + s                      c = a_m * s                          (ADD_HALF(a_m, s))
 *     j >  m, k_j = 1:   out_j = (a_j + s) + c                c = (a_j * s) + ((a_j + s) * c)      (ADD_FULL(c, a_j, s))
 *     j >  m, k_j = 0:   out_j = a_j + c                      c = a_j * c                          (ADD_FULL without b: a_j the LEFT operand)
 *     carry-out (optional, output index w) = the c left after j = w-1
 * Terms.  Let tn_j = k_j ? ts : 0 and C_{m-1} = 0.  Then T_j = ta_j + tn_j + C_{j-1} and C_j = ta_j * tn_j + (ta_j +
 * tn_j) * C_{j-1}.  The carry-out has C_{w-1} terms.  This is csgn_uint_arith's ADD formula with tb_j := tn_j.  Fresh a
 * and s: a + (s ? 1 : 0) has 2 terms in every plane and a carry of 1, 2w + 1 in all, for every width.
 * Order.  It is also that formula's order.  Plane j is [a_j | s (k_j = 1) | the entries of c_{j-1}].  Entry q of c_j,
 * for q < ta_j * tn_j, is term q / tn_j of a_j ANDed with term q % tn_j of s, which ends the walk.  Otherwise, with q' =
 * q - ta_j * tn_j, it is term q' / C_{j-1} of the concatenation a_j | s ANDed with entry q' % C_{j-1} of c_{j-1}.
 * In clear bits: where k_j = 1, c' = maj(a_j, s, c); where k_j = 0, c' = a_j * c.  An entry may hold several terms of
 * s: they pile up through (a_j + s) * c, and nothing cancels.
 * Derived operations add no words:
 *     a - (s ? k : 0) = a + (s ? (2^w - k) mod 2^w : 0), planes only: its carry is not a borrow
 *     increment and decrement where set are k = 1 and k = 2^w - 1 */
/* width + 1 counts into h_out_terms, the last the carry-out's (host only).  Returns 1, or 0 (h_out_terms not written) for
 * a width outside 1..32, k >= 2^width, a null pointer, t_sel or a plane of 0 terms, or a count of 2^62 or more. */
int csgn_uint_add_where_terms(uint64_t width, uint64_t k, uint64_t t_sel, const uint64_t *h_terms, uint64_t *h_out_terms);
/* The operation over `batch` elements.  h_planes and h_outs are HOST arrays of `width` device pointers: plane j takes
 * batch * h_terms[j] * dL words and output j batch * T_j * dL words.  d_carry takes batch * C_{w-1} * dL words, or is
 * NULL: the carry is then neither computed nor written.  Inputs may alias one another; d_sel may BE a plane of a.  No
 * output overlaps an input or another output.  Checks, in this order, the first that fails giving the status: n_bits;
 * the width and k; the host pointers; the term counts (CSGN_ERR_INVALID); every output's T * dL below 2^31 words per
 * element and batch times that below 2^60 (CSGN_ERR_UNSUPPORTED; computed without wrap-around); null device pointers,
 * among them d_sel where k != 0 (CSGN_ERR_INVALID); the device (CSGN_ERR_NO_DEVICE, no CPU fallback).  batch == 0
 * succeeds.  Nothing is allocated or launched before every check has passed.  On the caller's stream, asynchronous; one
 * launch for every shape within memory (k_uint_add_where) and graph-capturable.  The width stops at 32 here
 * because the kernel's arguments stay within 4 KB; certfhe/UInt.h composes wider integers. */
int csgn_uint_add_where(uint64_t n_bits, uint64_t batch, uint64_t width, uint64_t k,
                        const uint64_t *d_sel, uint64_t t_sel,
                        const uint64_t *const *h_planes, const uint64_t *h_terms,
                        uint64_t *const *h_outs, uint64_t *d_carry, void *stream);

/* ------------------------------------- the plane-by-plane operators of encrypted integers ---- */

/* a & b, a | b, a ^ b, ~a, select(s, a, b) and the mask s * a of ENCRYPTED integers, every plane in one launch: what
 * certfhe/UInt.h's operator&, operator|, operator^, operator~, select and keepWhere compute.
 * Inputs: a and b, integers of `width` = w planes (w in 1..64, bit 0 first) of `batch` elements, plane j uniform with
 * h_a_terms[j] = ta / h_b_terms[j] = tb terms per element, and d_sel, ONE batch of t_sel = ts terms per element.
 * Output plane j is the composition of the reference's operator+ (concatenation) and operator* (all-pairs AND, row i
 * = the left operand's term i against every term of the right one) the class operators make of plane j, word for
 * word, in the order of the Gates table above:
 *     op       plane j                                          terms
 *     AND      a_j * b_j                                        ta * tb
 *     OR       (a_j + b_j) + (a_j * b_j)                        ta + tb + ta * tb
 *     XOR      a_j + b_j                                        ta + tb
 *     NOT      a_j + ONE                                        ta + 1
 *     SELECT   (s * (a_j + b_j)) + b_j                          ts * (ta + tb) + tb
 *     KEEP     s * a_j   (the selector is the LEFT operand)     ts * ta
 * SELECT decrypts to s ? a : b and KEEP to s ? a : 0, element by element. */
enum { CSGN_UINT_BITWISE_AND = 1, CSGN_UINT_BITWISE_OR, CSGN_UINT_BITWISE_XOR,
       CSGN_UINT_BITWISE_NOT, CSGN_UINT_BITWISE_SELECT, CSGN_UINT_BITWISE_KEEP };
/* Terms per element of one output plane (host only); csgn_gate_terms' count for OR, NOT and MUX.  0 for an unknown op,
 * for a zero count of an operand the op reads (a: every op; b: AND, OR, XOR, SELECT; the selector: SELECT, KEEP), or
 * for a count of 2^62 or more.  The counts of operands the op does not read are ignored. */
uint64_t csgn_uint_bitwise_terms(int op, uint64_t t_sel, uint64_t t_a, uint64_t t_b);
/* Which form a csgn_uint_bitwise call of this shape takes under the calling thread's knobs (host only, a static
 * string): "k_uint_bitwise" (ONE kernel for every plane: a workgroup belongs to one plane, a lane writes one 16- or
 * 8-byte unit; its arguments hold the tables of all 64 planes, so a call is one launch, split by elements only at
 * knob "launch_blocks" and at HIP's limit of 2^32 lanes) or "planes" (csgn_mul_uniform's, csgn_add_uniform's and
 * csgn_gate_uniform's launchers plane by plane, each writing its output plane: one to three launches a plane).  Knob
 * "uint_bitwise_form" (-1 per shape, 0 planes, 1 the kernel) decides; left at -1, a forced knob "gate_fused" gives
 * the planes, and a shape of which one element of all planes does not fit one launch's lanes takes the planes
 * whatever the knob says.  The words are the same.  Per shape: DESIGN 4.31.  "" for an invalid shape (n_bits 0, an
 * unknown op, a width outside 1..64, a null pointer to counts the op reads, a bad term count). */
const char *csgn_uint_bitwise_kernel(uint64_t n_bits, int op, uint64_t batch, uint64_t width, uint64_t t_sel,
                                     const uint64_t *h_a_terms, const uint64_t *h_b_terms);
/* The operation over `batch` elements.  h_a, h_b, h_out: HOST arrays of `width` device pointers (plane j: batch * ta_j
 * * dL, batch * tb_j * dL and batch * T_j * dL words), d_sel: batch * ts * dL words.  The pointers and counts of an
 * operand the op does not read are not looked at and may be NULL / 0.  Inputs may alias one another in any way (a & a,
 * b_j == a_{j-1} after a public rotate, the selector a plane of a); no output overlaps an input or another output.
 * Checks, in this order, the first that fails giving the status: n_bits; op; width; the host arrays and the device
 * pointers in them and d_sel (CSGN_ERR_INVALID); the term counts (CSGN_ERR_INVALID); every plane's T * dL below 2^31
 * words per element and batch times that below 2^60 (CSGN_ERR_UNSUPPORTED; computed without wrap-around); the device
 * (CSGN_ERR_NO_DEVICE, no CPU fallback).  batch == 0 succeeds.  On the caller's stream, asynchronous,
 * graph-capturable; no scratch in either form. */
int csgn_uint_bitwise(uint64_t n_bits, int op, uint64_t batch, uint64_t width,
                      const uint64_t *d_sel, uint64_t t_sel,
                      const uint64_t *const *h_a, const uint64_t *h_a_terms,
                      const uint64_t *const *h_b, const uint64_t *h_b_terms,
                      uint64_t *const *h_out, void *stream);

/* ------------------------------------- a public matrix over F2 applied to an encrypted integer ---- */

/* csgn_uint_linear: a PUBLIC linear (affine) map over F2 of an ENCRYPTED integer, every output plane in one launch:
 * what certfhe/UInt.h's linearMap and parity compute -- SHA-2's sigma functions, xorshift steps, Gray codes, CRC steps,
 * AES MixColumns, a carry-less product with a public factor, a product with a public constant in GF(2^w), a masked
 * parity.  Over F2 a public matrix costs no multiplication: an output plane is a concatenation of input planes.
 * Inputs:
 *   - in_width uniform planes a_0 ... a_{in_width-1} (in_width in 1..64, bit 0 first), plane i of h_terms[i] = ta_i >= 1
 *     terms per element;
 *   - out_width rows (1..64): row j is the 64-bit mask M_j = h_rows[j] over the input planes (a bit at or above
 *     in_width: CSGN_ERR_INVALID);
 *   - `constant`, whose bit j adds ONE to plane j (a bit at or above out_width: CSGN_ERR_INVALID).
 * Output plane j is the left-nested sum (the reference's operator+: concatenation), ascending in i, of the a_i with bit
 * i of M_j set, followed by + ONE where constant_j = 1 (the form of NOT in the Gates table):
 *     plane j = ((a_{i1} + a_{i2}) + ...) + a_{im} [+ ONE]         T_j = sum over i in M_j of ta_i, + constant_j
 * A row with M_j = 0 is the one-term constant: ZERO (zero words) for constant_j = 0, ONE for 1; T_j = 1.  Rows may
 * repeat.  Input pointers may alias one another; no output overlaps an input or another output.
 * Nothing cancels on the device: what is public cancels on the host, in the matrix (certfhe/UInt.h's F2Matrix composes
 * two maps over F2 before anything runs). */
/* T_j of one row (host only).  0 for an in_width outside 1..64, a null pointer, a plane of 0 terms, a row bit at or above
 * in_width, a constant_bit other than 0 or 1, or a count of 2^62 or more. */
uint64_t csgn_uint_linear_terms(uint64_t in_width, const uint64_t *h_terms, uint64_t row, int constant_bit);
/* The decode by position (host only): the input plane *h_plane and the term *h_term of it that term q < T_j of the row
 * copies.  *h_plane = in_width means ONE and in_width + 1 means ZERO (*h_term = 0).  It runs the two functions the
 * kernel runs (the segment search and the s-th set bit of the mask; csgn_uint_linear.hip).  Returns 1, or 0 (nothing
 * written) for arguments csgn_uint_linear_terms refuses, q >= T_j or a null pointer. */
int csgn_uint_linear_decode(uint64_t in_width, const uint64_t *h_terms, uint64_t row, int constant_bit, uint64_t q,
                            uint64_t *h_plane, uint64_t *h_term);
/* How a call of this shape is cut under the calling thread's knob "launch_blocks" (host only, no device work).  The
 * grid is tile-major: a tile is G elements of ALL output planes, every plane's units of a tile rounded up to whole
 * 256-lane workgroups, and launches are cut at whole tiles only.
 *     h_plan[0]  bytes of the unit one lane writes when every pointer is 16-byte aligned: 16 for an even number of
 *                words per term, else 8 (a call with a pointer off alignment takes 8-byte units: twice the units, the
 *                same G rule)
 *     h_plan[1]  units per element over all output planes
 *     h_plan[2]  G, the elements per tile: (tile budget / units per element), at least 1 and at most `batch`
 *     h_plan[3]  tiles = ceil(batch / G)
 *     h_plan[4]  workgroups per tile
 *     h_plan[5]  launches (0 for batch == 0)
 *     h_plan[6]  the tile budget in units (DESIGN 4.36 says how it was chosen)
 *     h_plan[7]  plane groups: 1, unless ONE tile of all planes passes HIP's limit of 2^32 lanes a launch; the planes
 *                then go in that many runs of consecutive planes, each with launches of its own
 * The same checks as csgn_uint_linear, in its order, up to the sizes; it lets a caller ask for every refusal first. */
int csgn_uint_linear_plan(uint64_t n_bits, uint64_t batch, uint64_t in_width, const uint64_t *h_terms,
                          uint64_t out_width, const uint64_t *h_rows, uint64_t constant, uint64_t h_plan[8]);
/* The operation over `batch` elements.  h_in and h_out are HOST arrays of in_width / out_width device pointers: input
 * plane i takes batch * ta_i * dL words and output j batch * T_j * dL words.  Checks, in this order, the first that
 * fails giving the status: n_bits; the widths and the constant; the host arrays; row bits at or above in_width and the
 * term counts (CSGN_ERR_INVALID); every ta_i * dL and T_j * dL below 2^31 words per element and batch times that below
 * 2^60 (CSGN_ERR_UNSUPPORTED; computed without wrap-around); null device pointers (CSGN_ERR_INVALID); the device
 * (CSGN_ERR_NO_DEVICE, no CPU fallback).  batch == 0 succeeds.  On the caller's stream, asynchronous and
 * graph-capturable: k_uint_linear, one launch for every shape csgn_uint_linear_plan gives one; no
 * scratch, no allocation, no synchronisation. */
int csgn_uint_linear(uint64_t n_bits, uint64_t batch, uint64_t in_width, const uint64_t *const *h_in,
                     const uint64_t *h_terms, uint64_t out_width, const uint64_t *h_rows, uint64_t constant,
                     uint64_t *const *h_out, void *stream);

/* ------------------------------------- sums of comparisons against public constants ---- */

/* csgn_uint_plain_sum: sums over F2 of comparisons of ONE ENCRYPTED integer against PUBLIC constants, every output
 * plane in one launch: what certfhe/UInt.h's inRange, inRanges, isIn, stepFunction, bucketOf and lookupSparse compute.
 * A range lo <= a <= hi is [a < hi + 1] + [a < lo]; membership in a set is the sum of the disjoint [a == k_i]; bit j of a
 * step function is the sum of [a < t_i] over the thresholds where bit j of the value changes.  None of them multiplies
 * beyond what each comparison multiplies.
 * Inputs:
 *   - width uniform planes a_0 ... a_{w-1} (width in 1..64, bit 0 first), plane j of h_terms[j] = t_j >= 1 terms per
 *     element;
 *   - n_out output planes (1..64).  The entries of plane x are h_first[x] .. h_first[x+1] - 1 (h_first[0] = 0, h_first
 *     non-descending, n_out + 1 values) of the parallel host arrays h_cmp[] (CSGN_UINT_PLAIN_EQ .. GE) and h_k[] (each
 *     below 2^width);
 *   - `constant`, whose bit x adds ONE to plane x (a bit at or above n_out: CSGN_ERR_INVALID).
 * Output plane x is the left-nested sum (the reference's operator+: concatenation) of its entries' csgn_uint_plain
 * results, in order and word for word -- the ONE that NE / LE / GE append and the one-term ZERO of LT k = 0 and
 * GT k = 2^w - 1 included --, followed by + ONE where constant_x = 1:
 *     plane x = ((P(cmp_i1, k_i1) + P(cmp_i2, k_i2)) + ...) + P(cmp_im, k_im) [+ ONE]
 *     T_x = sum over the plane's entries of csgn_uint_plain_terms(cmp_i, width, k_i, h_terms), + constant_x
 * A plane with no entry is the one-term constant: ZERO (zero words) for constant_x = 0, ONE for 1; T_x = 1
 * (csgn_uint_linear's rule for an empty row).  Input pointers may alias one another; no output overlaps an input or
 * another output.  Nothing cancels on the device: an entry named twice is written twice (and cancels over F2 only at
 * decryption); certfhe/UInt.h sorts and deduplicates on the host. */
/* T of ONE plane of n_entries entries (host only).  0 for anything csgn_uint_plain_terms refuses in an entry, a null
 * array (h_cmp and h_k may be null when n_entries = 0), a constant_bit other than 0 or 1, or a count of 2^62 or more. */
uint64_t csgn_uint_plain_sum_terms(uint64_t width, const uint64_t *h_terms, uint64_t n_entries, const int *h_cmp,
                                   const uint64_t *h_k, int constant_bit);
/* The decode by position (host only): term q < T of ONE plane is the AND of *h_n_factors (1..64) terms, factor f being
 * term h_level_term[f] of input plane h_level_plane[f]; plane `width` means ONE and `width + 1` means ZERO (term 0):
 * the ONE of a factor a_j + ONE, the ONE an entry or the plane appends, the ZERO of an entry or of an empty plane.
 * Factors come from the top plane down.  It runs the functions the kernel runs: the entry search (sum_entry,
 * csgn_uint_plain_sum.hip) over the entries' first terms, then the chain walk (chain_walk_each, csgn_device.h) over
 * the entry's level record.  Returns 1, or 0 (nothing written) for arguments csgn_uint_plain_sum_terms refuses, more
 * than 65536 entries, a plane of 2^31 terms or more, q >= T or a null pointer. */
int csgn_uint_plain_sum_decode(uint64_t width, const uint64_t *h_terms, uint64_t n_entries, const int *h_cmp,
                               const uint64_t *h_k, int constant_bit, uint64_t q, uint64_t h_level_plane[65],
                               uint64_t h_level_term[65], uint64_t *h_n_factors);
/* How a call of this shape is cut under the calling thread's knob "launch_blocks" (host only, no device work).  A lane
 * item is (element, plane, run of up to 16 consecutive terms of ONE entry, unit); the plane's constant is a run of its
 * own.  The grid is plane-major: every plane's items of the launch's elements rounded up to whole 256-lane workgroups.
 * Launches are cut at elements: ne elements go where  sum over the planes of ceil(ne * items_x / 256)  workgroups fit,
 * bounded by  ne * items / 256 + planes  (one element goes whole whatever the knob says).
 *     h_plan[0]  bytes of the unit one lane writes when every pointer is 16-byte aligned: 16 for an even number of
 *                words per term, else 8 (a call with a pointer off alignment takes 8-byte units: twice the units)
 *     h_plan[1]  lane items per element over all output planes
 *     h_plan[2]  plane groups: 1, unless ONE element of all planes passes HIP's limit of 2^32 lanes a launch; the planes
 *                then go in that many runs of consecutive planes, each with launches of its own
 *     h_plan[3]  launches (0 for batch == 0)
 *     h_plan[4]  elements of the first launch
 *     h_plan[5]  workgroups of the first launch
 * The same checks as csgn_uint_plain_sum_create, in its order, then h_plan, then the sizes of csgn_uint_plain_sum. */
int csgn_uint_plain_sum_launches(uint64_t n_bits, uint64_t batch, uint64_t width, const uint64_t *h_terms,
                                 uint64_t n_out, const uint64_t *h_first, const int *h_cmp, const uint64_t *h_k,
                                 uint64_t constant, uint64_t h_plan[6]);
/* The plan of one shape: every entry's level record (base, top, cut, the zero / neg flags, the radix-1 mask, pend[],
 * the FastDivs and T, with the entry's first run and first term in its plane) built from the chain of csgn_uint_plain
 * and uploaded once, synchronously.  Checks, in this order: `plan`; width; n_out and the constant; h_terms and h_first,
 * h_first[0] = 0 and non-descending, h_cmp and h_k where there is an entry (CSGN_ERR_INVALID); more than 65536 entries
 * (CSGN_ERR_UNSUPPORTED); the planes' term counts, the comparisons and constants of the entries, the term counts of the
 * results (CSGN_ERR_INVALID); an output plane of 2^31 terms per element or more (CSGN_ERR_UNSUPPORTED); the device
 * (CSGN_ERR_NO_DEVICE, no CPU fallback).  Release with csgn_uint_plain_sum_destroy (null is ignored).  A plan is
 * immutable: any number of threads and streams may launch from it. */
typedef struct csgn_uint_plain_sum_plan csgn_uint_plain_sum_plan;
int csgn_uint_plain_sum_create(uint64_t width, const uint64_t *h_terms, uint64_t n_out, const uint64_t *h_first,
                               const int *h_cmp, const uint64_t *h_k, uint64_t constant,
                               csgn_uint_plain_sum_plan **plan);
/* T_x of plane x of the plan; 0 for a null plan or x >= n_out */
uint64_t csgn_uint_plain_sum_plan_terms(const csgn_uint_plain_sum_plan *plan, uint64_t x);
void csgn_uint_plain_sum_destroy(csgn_uint_plain_sum_plan *plan);
/* The operation over `batch` elements.  h_planes and h_out are HOST arrays of width / n_out device pointers: input
 * plane j takes batch * t_j * dL words and output x batch * T_x * dL words.  Checks, in this order: n_bits; the host
 * arrays; the plan (a null plan is CSGN_ERR_NO_DEVICE where there is no device -- no plan exists there -- and
 * CSGN_ERR_INVALID otherwise); every t_j * dL and T_x * dL below 2^31 words per element and batch times that below
 * 2^60 (CSGN_ERR_UNSUPPORTED); null device pointers, all `width` inputs and n_out outputs (CSGN_ERR_INVALID); the
 * device (CSGN_ERR_NO_DEVICE, no CPU fallback).  batch == 0 succeeds.  On the caller's stream, asynchronous and
 * graph-capturable: k_uint_plain_sum, one launch for every shape csgn_uint_plain_sum_launches gives one;
 * no scratch, no allocation, no synchronisation. */
int csgn_uint_plain_sum(const csgn_uint_plain_sum_plan *plan, uint64_t n_bits, uint64_t batch,
                        const uint64_t *const *h_planes, uint64_t *const *h_out, void *stream);

/* ------------------------------------- a public bilinear form of two encrypted integers ---- */

/* csgn_uint_bilinear: a PUBLIC bilinear form over F2 of TWO ENCRYPTED integers, every output plane in one launch: what
 * certfhe/UInt.h's bilinearMap, clmul, clmulWide, gfMul and dotBits compute -- the carry-less product of GHASH /
 * POLYVAL and of every polynomial MAC, the product in GF(2^w) (AES's inversion, Reed-Solomon, Shamir shares over
 * GF(256)), a secret bit matrix applied to a secret vector, parity(a & b).  No carry exists: an output bit is a sum
 * over F2 of products of one bit of a and one bit of b.
 * Inputs:
 *   - wa uniform planes a_0 ... a_{wa-1} (wa in 1..64, bit 0 first), plane i of h_ta[i] = ta_i >= 1 terms per element,
 *     and wb planes b_0 ... b_{wb-1} (wb in 1..64) of h_tb[l] = tb_l >= 1;
 *   - n_out output planes (1..64).  The entries of plane x are h_first[x] .. h_first[x+1] - 1 (h_first[0] = 0, h_first
 *     non-descending, n_out + 1 values) of the parallel host arrays h_left[] (each below wa) and h_right[] (each below
 *     wb);
 *   - `constant`, whose bit x adds ONE to plane x (a bit at or above n_out: CSGN_ERR_INVALID).
 * Output plane x is the left-nested sum (the reference's operator+: concatenation) of the products (the reference's
 * operator*: every pair of terms ANDed, the left term slow) of its entries, in the order given, followed by + ONE where
 * constant_x = 1:
 *     plane x = ((a_l1 * b_r1 + a_l2 * b_r2) + ...) + a_lm * b_rm [+ ONE]
 *     T_x = sum over the plane's entries of ta_left * tb_right, + constant_x
 * A plane with no entry is the one-term constant: ZERO (zero words) for constant_x = 0, ONE for 1; T_x = 1
 * (csgn_uint_linear's rule for an empty row).  Input pointers may alias in any way -- a and b may be the same planes,
 * which gives squares --; no output overlaps an input or another output.  Nothing cancels on the device: an entry
 * named twice is written twice (and cancels over F2 only at decryption); certfhe/UInt.h's F2Bilinear sorts and cancels
 * on the host. */
/* T of ONE plane of n_entries entries (host only).  0 for a width outside 1..64, a null array (h_left and h_right may
 * be null when n_entries = 0), a plane of 0 terms or 2^62 or more, an entry at or above its width, a constant_bit other
 * than 0 or 1, or a count of 2^62 or more (computed without wrap-around). */
uint64_t csgn_uint_bilinear_terms(uint64_t wa, const uint64_t *h_ta, uint64_t wb, const uint64_t *h_tb,
                                  uint64_t n_entries, const uint64_t *h_left, const uint64_t *h_right, int constant_bit);
/* The decode by position (host only): term q < T of ONE plane is term *h_left_term of a_left ANDed with term
 * *h_right_term of b_right of entry *h_entry.  *h_entry = n_entries means ONE and n_entries + 1 means ZERO (both terms
 * 0).  It runs the two functions the kernel runs (bilinear_entry: one division where all ta are equal and all tb are
 * equal, else the search over the entries' first terms; bilinear_split; csgn_uint_bilinear.hip).  Returns 1, or 0
 * (nothing written) for arguments csgn_uint_bilinear_terms refuses, more than 262144 entries, a plane of 2^31 terms or
 * more, q >= T or a null pointer. */
int csgn_uint_bilinear_decode(uint64_t wa, const uint64_t *h_ta, uint64_t wb, const uint64_t *h_tb, uint64_t n_entries,
                              const uint64_t *h_left, const uint64_t *h_right, int constant_bit, uint64_t q,
                              uint64_t *h_entry, uint64_t *h_left_term, uint64_t *h_right_term);
/* How a call of this shape is cut under the calling thread's knob "launch_blocks" (host only, no device work).  The
 * grid is tile-major: a tile is G elements of ALL output planes, and the stream of a tile is (plane, element, term,
 * unit) with the unit fastest, ge * h_plan[1] units for a tile of ge elements.  Workgroup b of a launch belongs to tile
 * b / S (S = h_plan[4]) of the launch and is its workgroup s = b % S: lane l writes the positions s * chunk + l,
 * + 256, ... below min((s + 1) * chunk, the tile's units).  Launches are cut at whole tiles only: max(1, launch_blocks
 * / S) tiles each.
 *     h_plan[0]   bytes of the unit one lane writes when every pointer is 16-byte aligned: 16 for an even number of
 *                 words per term, else 8 (a call with a pointer off alignment takes 8-byte units: twice the units, the
 *                 same rules)
 *     h_plan[1]   units per element over all output planes
 *     h_plan[2]   G, the elements per tile.  Staged: as many as h_plan[11] bytes hold the operand units of (h_plan[10]
 *                 units an element); else (tile budget / units per element); at least 1, at most `batch`, and no more
 *                 than keep a tile within 2^31 units
 *     h_plan[3]   tiles = ceil(batch / G) (0 for batch == 0)
 *     h_plan[4]   S, the workgroups per tile: (G * units per element / least), at least 1, where a workgroup walks at
 *                 `least` 2048 units and, staged, 4 times the units it stages (G * h_plan[10]); summed over the plane
 *                 groups
 *     h_plan[5]   launches (0 for batch == 0)
 *     h_plan[6]   workgroups of the first launch (0 for batch == 0)
 *     h_plan[7]   plane groups: 1, unless ONE element of all planes passes 2^31 units; G is then 1 and the planes go in
 *                 that many runs of consecutive planes, each a stream and a launch sequence of its own
 *     h_plan[8]   1 when the shape is STAGED: every workgroup copies its tile's operand units to LDS once and reads
 *                 them there.  A shape is staged when one element's operand units fit h_plan[11] bytes and the form
 *                 writes at least twice the units it reads; else both operand units of a written unit are loaded from
 *                 memory.  A function of the shape, not a knob
 *     h_plan[9]   chunk, the units a workgroup walks: the tile's G * units per element in S even parts, rounded up
 *                 to a multiple of 256 (of the first plane group)
 *     h_plan[10]  operand units per element: (sum of ta + sum of tb) * units per term
 *     h_plan[11]  the LDS budget for operand units, in bytes
 * The same checks as csgn_uint_bilinear_create, in its order, then h_plan, then the sizes of csgn_uint_bilinear. */
int csgn_uint_bilinear_launches(uint64_t n_bits, uint64_t batch, uint64_t wa, const uint64_t *h_ta, uint64_t wb,
                                const uint64_t *h_tb, uint64_t n_out, const uint64_t *h_first, const uint64_t *h_left,
                                const uint64_t *h_right, uint64_t constant, uint64_t h_plan[12]);
/* The plan of one shape: the planes' term counts and divisors, the entry table and, per plane, the entries' first
 * terms, uploaded once, synchronously.  Checks, in this order: `plan`; wa; wb; n_out and the constant; h_ta, h_tb and
 * h_first, h_first[0] = 0 and non-descending, h_left and h_right where there is an entry (CSGN_ERR_INVALID); more than
 * 262144 entries (CSGN_ERR_UNSUPPORTED); the planes' term counts, the entries' indices, the term counts of the output
 * planes (CSGN_ERR_INVALID); an output plane of 2^31 terms per element or more (CSGN_ERR_UNSUPPORTED); the device
 * (CSGN_ERR_NO_DEVICE, no CPU fallback).  Release with csgn_uint_bilinear_destroy (null is ignored).  A plan is
 * immutable: any number of threads and streams may launch from it. */
typedef struct csgn_uint_bilinear_plan csgn_uint_bilinear_plan;
int csgn_uint_bilinear_create(uint64_t wa, const uint64_t *h_ta, uint64_t wb, const uint64_t *h_tb, uint64_t n_out,
                              const uint64_t *h_first, const uint64_t *h_left, const uint64_t *h_right,
                              uint64_t constant, csgn_uint_bilinear_plan **plan);
/* T_x of plane x of the plan; 0 for a null plan or x >= n_out */
uint64_t csgn_uint_bilinear_plan_terms(const csgn_uint_bilinear_plan *plan, uint64_t x);
void csgn_uint_bilinear_destroy(csgn_uint_bilinear_plan *plan);
/* The operation over `batch` elements.  h_a, h_b and h_out are HOST arrays of wa / wb / n_out device pointers: plane i
 * of a takes batch * ta_i * dL words, plane l of b batch * tb_l * dL and output x batch * T_x * dL words.  Checks, in
 * this order: n_bits; the host arrays; the plan (a null plan is CSGN_ERR_NO_DEVICE where there is no device -- no plan
 * exists there -- and CSGN_ERR_INVALID otherwise); every ta_i * dL, tb_l * dL and T_x * dL below 2^31 words per element
 * and batch times that below 2^60 (CSGN_ERR_UNSUPPORTED); null device pointers, a, then b, then the outputs
 * (CSGN_ERR_INVALID); the device (CSGN_ERR_NO_DEVICE, no CPU fallback).  batch == 0 succeeds.  On the caller's stream,
 * asynchronous and graph-capturable: k_uint_bilinear, one launch for every shape
 * csgn_uint_bilinear_launches gives one; no scratch, no allocation, no synchronisation. */
int csgn_uint_bilinear(const csgn_uint_bilinear_plan *plan, uint64_t n_bits, uint64_t batch,
                       const uint64_t *const *h_a, const uint64_t *const *h_b, uint64_t *const *h_out, void *stream);

/* ------------------------------------- a public polynomial over F2 of encrypted planes ---- */

/* csgn_uint_poly: a PUBLIC polynomial over F2 of ENCRYPTED planes, sparse, of mixed degree up to 8, every output plane
 * in one launch: SHA-2's Ch(e,f,g) = ef + eg + g and Maj(a,b,c) = ab + ac + bc, Keccak's chi a + c + bc, a Simon
 * round, Trivium and Grain updates, a full adder's carry, a k-way AND, an S-box ANF on wide words.  It covers what lies
 * between csgn_uint_linear (degree 1), csgn_uint_bilinear (pure degree 2 of two integers) and csgn_uint_lut (dense, at
 * most 16 input bits).  No carry exists: an output bit is a sum over F2 of products of input bits.
 * Inputs:
 *   - n_in uniform input planes (1..256), plane i of h_terms[i] = t_i >= 1 terms per element.  The caller concatenates
 *     its integers' planes: the ABI knows nothing of operands;
 *   - n_out output planes (1..64).  The monomials of plane x are h_first[x] .. h_first[x+1] - 1 (h_first[0] = 0,
 *     h_first non-descending, n_out + 1 values);
 *   - monomial m has the factors h_factor[h_mfirst[m] .. h_mfirst[m+1] - 1] (h_mfirst[0] = 0, h_first[n_out] + 1
 *     values), each below n_in; its degree h_mfirst[m+1] - h_mfirst[m] is 1..8;
 *   - `constant`, whose bit x adds ONE to plane x (a bit at or above n_out: CSGN_ERR_INVALID).
 * Output plane x is the left-nested sum (the reference's operator+: concatenation) of its monomials in the order given,
 * followed by + ONE where constant_x = 1; a monomial is the left-nested product (the reference's operator*: every pair
 * of terms ANDed, the left term slow) of its factors in the order given:
 *     plane x = ((M_1 + M_2) + ...) + M_m [+ ONE]
 *     M       = ((p_f1 * p_f2) * ...) * p_fd         prod t_f terms, the first factor's term index slowest
 *     T_x     = sum over the plane's monomials of prod t_f, + constant_x
 * A plane with no monomial is the one-term constant: ZERO (zero words) for constant_x = 0, ONE for 1; T_x = 1
 * (csgn_uint_linear's rule for an empty row).  Input pointers may alias in any way; no output overlaps an input or
 * another output.  Nothing cancels on the device: a monomial named twice is written twice (and cancels over F2 only at
 * decryption), and a factor named twice inside a monomial is multiplied with itself, t^2 terms. */
/* T of ONE plane of n_monomials monomials (host only); monomial m has the factors h_factor[h_mfirst[m] ..
 * h_mfirst[m+1] - 1], h_mfirst[0] being any offset into h_factor, so a plane of a plan's arrays is h_mfirst +
 * h_first[x] with the plan's h_factor.  0 for n_in outside 1..256, a null array (h_mfirst and h_factor may be null when
 * n_monomials = 0), an input plane of 0 terms or 2^62 or more, a degree outside 1..8, a factor at or above n_in, a
 * constant_bit other than 0 or 1, or a count of 2^62 or more (computed without wrap-around). */
uint64_t csgn_uint_poly_terms(uint64_t n_in, const uint64_t *h_terms, uint64_t n_monomials, const uint64_t *h_mfirst,
                              const uint64_t *h_factor, int constant_bit);
/* The decode by position (host only): term q < T of ONE plane is the AND, over the factors j < degree of monomial
 * *h_monomial, of term h_factor_terms[j] of that factor's plane (8 values are written, 0 at and past the degree).
 * *h_monomial = n_monomials means ONE and n_monomials + 1 means ZERO.  It runs the two functions the kernel runs
 * (poly_monomial: one division where every input plane has one term count and every monomial one degree, else the
 * search over the monomials' first terms; poly_split: the mixed-radix division; csgn_uint_poly.hip).  Returns 1, or 0
 * (nothing written) for arguments csgn_uint_poly_terms refuses, more than 262144 monomials, a plane of 2^31 terms or
 * more, q >= T or a null pointer. */
int csgn_uint_poly_decode(uint64_t n_in, const uint64_t *h_terms, uint64_t n_monomials, const uint64_t *h_mfirst,
                          const uint64_t *h_factor, int constant_bit, uint64_t q, uint64_t *h_monomial,
                          uint64_t h_factor_terms[8]);
/* How a call of this shape is cut under the calling thread's knob "launch_blocks" (host only, no device work).  The
 * grid, the tiles, the chunks and the cut into launches are csgn_uint_bilinear_launches', figure for figure:
 *     h_plan[0]   bytes of the unit one lane writes when every pointer is 16-byte aligned: 16 for an even number of
 *                 words per term, else 8 (a call with a pointer off alignment takes 8-byte units)
 *     h_plan[1]   units per element over all output planes
 *     h_plan[2]   G, the elements per tile.  Staged: as many as h_plan[11] bytes hold the operand units of (h_plan[10]
 *                 units an element); else (262144 / units per element); at least 1, at most `batch`, and no more than
 *                 keep a tile within 2^31 units
 *     h_plan[3]   tiles = ceil(batch / G) (0 for batch == 0)
 *     h_plan[4]   S, the workgroups per tile: (G * units per element / least), at least 1, where a workgroup walks at
 *                 `least` 2048 units and, staged, 4 times the units it stages (G * h_plan[10]); summed over the plane
 *                 groups
 *     h_plan[5]   launches (0 for batch == 0): max(1, launch_blocks / S) tiles each, cut at whole tiles only
 *     h_plan[6]   workgroups of the first launch (0 for batch == 0)
 *     h_plan[7]   plane groups: 1, unless ONE element of all planes passes 2^31 units; G is then 1 and the planes go in
 *                 that many runs of consecutive planes, each a stream and a launch sequence of its own
 *     h_plan[8]   1 when the shape is STAGED: one element's operand units fit h_plan[11] bytes and the form writes at
 *                 least twice the units it reads; every workgroup then copies its tile's operand units to LDS once
 *     h_plan[9]   chunk, the units a workgroup walks: G * units per element in S even parts, rounded up to a multiple
 *                 of 256 (of the first plane group)
 *     h_plan[10]  operand units per element: (sum of t_i) * units per term
 *     h_plan[11]  the LDS budget for operand units, in bytes
 *     h_plan[12]  1 when a lane finds its monomial by one division: every input plane has one term count t, every
 *                 monomial of the plan one degree d, and t^d is below 2^31; else by the search
 *     h_plan[13]  how a lane finds the factors' term indices: 0 nothing is divided (every t_i = 1), 1 one shared
 *                 divisor (every t_i equal), 2 the planes' divisors from the plan
 * The same checks as csgn_uint_poly_create, in its order, then h_plan, then the sizes of csgn_uint_poly. */
int csgn_uint_poly_launches(uint64_t n_bits, uint64_t batch, uint64_t n_in, const uint64_t *h_terms, uint64_t n_out,
                            const uint64_t *h_first, const uint64_t *h_mfirst, const uint64_t *h_factor,
                            uint64_t constant, uint64_t h_plan[14]);
/* The plan of one shape: the planes' term counts and divisors and one 16-byte record per monomial, uploaded once,
 * synchronously.  Checks, in this order: `plan`; n_in; n_out and the constant; h_terms and h_first, h_first[0] = 0 and
 * non-descending, h_mfirst and h_factor where there is a monomial (CSGN_ERR_INVALID); more than 262144 monomials
 * (CSGN_ERR_UNSUPPORTED); the input planes' term counts, h_mfirst[0] = 0, every degree and every factor, the term
 * counts of the output planes (CSGN_ERR_INVALID); an output plane of 2^31 terms per element or more
 * (CSGN_ERR_UNSUPPORTED); the device (CSGN_ERR_NO_DEVICE, no CPU fallback).  Release with csgn_uint_poly_destroy (null
 * is ignored).  A plan is immutable: any number of threads and streams may launch from it. */
typedef struct csgn_uint_poly_plan csgn_uint_poly_plan;
int csgn_uint_poly_create(uint64_t n_in, const uint64_t *h_terms, uint64_t n_out, const uint64_t *h_first,
                          const uint64_t *h_mfirst, const uint64_t *h_factor, uint64_t constant,
                          csgn_uint_poly_plan **plan);
/* T_x of plane x of the plan; 0 for a null plan or x >= n_out */
uint64_t csgn_uint_poly_plan_terms(const csgn_uint_poly_plan *plan, uint64_t x);
void csgn_uint_poly_destroy(csgn_uint_poly_plan *plan);
/* The operation over `batch` elements.  h_in and h_out are HOST arrays of n_in / n_out device pointers: input plane i
 * takes batch * t_i * dL words and output x batch * T_x * dL words.  Checks, in this order: n_bits; the host arrays; the
 * plan (a null plan is CSGN_ERR_NO_DEVICE where there is no device -- no plan exists there -- and CSGN_ERR_INVALID
 * otherwise); every t_i * dL and T_x * dL below 2^31 words per element and batch times that below 2^60
 * (CSGN_ERR_UNSUPPORTED); null device pointers, the inputs, then the outputs (CSGN_ERR_INVALID); the device
 * (CSGN_ERR_NO_DEVICE, no CPU fallback).  batch == 0 succeeds.  On the caller's stream, asynchronous and
 * graph-capturable: k_uint_poly, one launch for every shape csgn_uint_poly_launches gives one; no scratch,
 * no allocation, no synchronisation. */
int csgn_uint_poly(const csgn_uint_poly_plan *plan, uint64_t n_bits, uint64_t batch, const uint64_t *const *h_in,
                   uint64_t *const *h_out, void *stream);

/* ------------------------------------- one-bit batches decrypted into one word per element ---- */

/* n_planes one-bit batches of `batch` elements decrypted in ONE pass into one 64-bit word per element: what
 * certfhe/UInt.h's UIntBatch::decrypt and decryptPacked compute.
 *     bit j of d_values[e] = Dec(element e of plane j) = XOR over the element's terms of (the term covers the key mask)
 *     bits n_planes .. 63 are 0; an element of 0 terms gives 0
 * Every word of d_values[0 .. batch) is written whatever it held before, and nothing beside them.  The planes need not
 * be an integer's: any list of one-bit batches of one count packs this way (a carry, a membership bit, the outputs of
 * a compare-exchange).  Plane j is uniform with h_terms[j] >= 1 terms per element (batch * h_terms[j] * dL words), or,
 * with h_terms[j] == 0, ragged: h_offsets[j] are its CSR term offsets on the device (batch + 1 words, offsets[0] = 0),
 * h_total_terms[j] = offsets[batch] and h_max_terms[j] a bound on the terms of ONE element (csgn_decrypt_ragged_bounded's
 * rules: a bound that does not hold is the caller's error; one that is not tight costs nothing).  h_offsets, h_total_terms and h_max_terms are read only at ragged planes and may be NULL when there are
 * none.  d_mask is the dL-word key mask (csgn_key_mask).  The call takes no scratch: no hit bitmap and no partial
 * parity go through HBM.
 * One kernel, k_uint_decrypt, reads every term of every plane exactly once: a workgroup owns a range of elements for ALL
 * planes and writes their words with plain stores.  Only an element of a uniform plane with more terms than knob
 * "uint_decrypt_chunk" (0: by shape, 1024; never above 4096) is cut into chunks, each of which XORs one bit into the
 * word with a 64-bit atomic; in that form, and only in it, a zero fill of d_values (a kernel) runs first.  A ragged
 * plane is never cut, which is why its bound may not pass 4096 terms (decrypt such a plane with
 * csgn_decrypt_ragged_bounded).  Knob "launch_blocks" or the HIP grid limit may split the kernel into several launches.
 * Checks, in this order, the first that fails giving the status, all of them before any device call: n_bits
 * (CSGN_ERR_INVALID at 0, CSGN_ERR_UNSUPPORTED past 16 KiB a term); n_planes in 1..64 and batch >= 1; the host pointers
 * h_planes and h_terms; for every ragged plane h_offsets, h_total_terms and h_max_terms present and
 * batch * max_terms >= total_terms (CSGN_ERR_INVALID); every plane below 2^31 words per element and 2^60 per batch
 * (CSGN_ERR_UNSUPPORTED; computed without wrap-around); a ragged bound above 4096 (CSGN_ERR_UNSUPPORTED); the device
 * (CSGN_ERR_NO_DEVICE, no CPU fallback); null device pointers (CSGN_ERR_INVALID; the words of a ragged plane of no terms
 * may be NULL).  On the caller's stream, asynchronous, graph-capturable. */
int csgn_uint_decrypt(uint64_t n_bits, uint64_t batch, uint64_t n_planes, const uint64_t *const *h_planes,
                      const uint64_t *h_terms, const uint64_t *const *h_offsets, const uint64_t *h_total_terms,
                      const uint64_t *h_max_terms, const uint64_t *d_mask, uint64_t *d_values, void *stream);
/* Which launches a csgn_uint_decrypt call of this shape makes under the calling thread's knobs (host only, a static
 * string): "k_uint_decrypt" (every plane owned: plain stores, no atomics) or "k_zero_words+k_uint_decrypt" (some
 * uniform plane has more terms than the chunk and is cut).  h_terms as above (0: ragged, never cut).  "" for an invalid
 * shape (n_bits 0, batch 0, n_planes outside 1..64, a null pointer). */
const char *csgn_uint_decrypt_kernel(uint64_t n_bits, uint64_t batch, uint64_t n_planes, const uint64_t *h_terms);

/* ------------------------------------- shifts, rotates and per-element reads by encrypted amounts ---- */

/* An encrypted integer shifted or rotated by an ENCRYPTED distance, or an array that belongs to the element read at the
 * element's ENCRYPTED index.  Index: index_width = v planes x_0..x_{v-1} (bit 0 first, v in 1..16) of `batch` elements,
 * plane k uniform with s_k terms per element.  Source: `width` = w planes a_0..a_{w-1} (1..64), EVERY one uniform with
 * the same t terms per element; of `batch` elements, or, for EACH, of batch * n elements (element e's array is the
 * elements e * n .. e * n + n - 1).  Output: w planes of `batch` elements.  A fixed composition of the reference's
 * operator+ / operator* with ONE, element e with element e:
 *     out_j = ((EQ(x, 0) * a_{src(j,0)}) + (EQ(x, 1) * a_{src(j,1)})) + ... + (EQ(x, rows_j - 1) * a_{src(j,rows_j-1)})
 *     EQ(x, r)   csgn_uint_plain's EQ row with k = r, the LEFT operand of every product, exactly as in csgn_uint_read
 *     op                    rows_j              src(j, r)                         decrypts to
 *     CSGN_UINT_PICK_SHL    min(j + 1, 2^v)     plane j - r                       (a << x) mod 2^w, 0 where x >= w
 *     CSGN_UINT_PICK_SHR    min(w - j, 2^v)     plane j + r                       a >> x, 0 where x >= w
 *     CSGN_UINT_PICK_ROTL   2^v                 plane (j - r) mod w               a rotated left by x mod w
 *     CSGN_UINT_PICK_ROTR   2^v                 plane (j + r) mod w               a rotated right by x mod w
 *     CSGN_UINT_PICK_EACH   n = `rows`          plane j of element e * n + r      row x of element e's array, 0 where x >= n
 * `rows` is n (1 <= n <= 2^v) for EACH and must be 0 for the shifts and rotates.
 * Terms of output j: t * E_j,  E_j = csgn_uint_read_terms(v, s, rows_j).  Fresh planes: the top plane of an 8-bit SHL by
 * a 3-bit distance has 27 terms, every plane of a 32-bit rotate by 5 bits 243.
 * Term order: csgn_uint_read's -- term q * t + c is (entry q of the E stream of rows_j rows) & (term c of the source);
 * rows are concatenated ascending, so the stream of a shorter output is a prefix of the longest one's. */
enum csgn_uint_pick_op {
    CSGN_UINT_PICK_SHL = 1,
    CSGN_UINT_PICK_SHR = 2,
    CSGN_UINT_PICK_ROTL = 3,
    CSGN_UINT_PICK_ROTR = 4,
    CSGN_UINT_PICK_EACH = 5
};
/* E_j (host only); 0 for an unknown op, index_width outside 1..16, width outside 1..64, j >= width, rows != 0 for a
 * shift or rotate, rows outside 1..2^index_width for EACH, a null pointer, an index plane of 0 terms or a count of 2^62
 * or more. */
uint64_t csgn_uint_pick_terms(int op, uint64_t index_width, const uint64_t *h_index_terms, uint64_t width, uint64_t rows,
                              uint64_t j);
/* Which form a csgn_uint_pick call of this shape takes (host only, a static string): "k_uint_pick" (one kernel writes
 * every output plane, planes read in place) or "composed" (per row r: csgn_uint_plain's EQ into a temporary the calling
 * thread keeps (csgn_uint_addk's rules for its composed form), for EACH csgn_gather_planes of the elements e * n + r --
 * the list e * n is uploaded, and waited for, once a call --, then csgn_mul_uniform into r's slice of every output that
 * has the row).  Knob "uint_pick_fused" (-1 per shape, 0 / 1 forced) decides; the words are the same.  Per shape: fused
 * for every shape (no shape is measured in favour of the composed form; EACH with batch * n of 2^32 or more is fused
 * whatever the knob says: the gather's counts stop there).  "" for an invalid shape.  Inside the fused form, knob
 * "uint_pick_stage" (-1 per shape, 0 / 1 forced) chooses whether a workgroup copies its slice of the source planes into
 * LDS (fresh index planes, where the slice fits; per shape: it does) or reads it with plain global loads; same words. */
const char *csgn_uint_pick_kernel(uint64_t n_bits, int op, uint64_t batch, uint64_t index_width,
                                  const uint64_t *h_index_terms, uint64_t width, uint64_t rows, uint64_t terms);
/* The fused form's tile for this shape (host only), for tests and tools: h_plan[0..3] = elements per workgroup, units of
 * a unit slice, E-stream entries a workgroup decodes (QP: workgroup part p owns entries [p * QP, (p + 1) * QP) of the
 * longest output's stream) and the number of such parts.  wide_units: nonzero for the 16-byte-unit kernel (taken when
 * dL is even and every pointer is 16-byte aligned).  CSGN_ERR_INVALID for an invalid shape or an empty batch. */
int csgn_uint_pick_plan(uint64_t n_bits, int op, uint64_t batch, uint64_t index_width, const uint64_t *h_index_terms,
                        uint64_t width, uint64_t rows, uint64_t terms, int wide_units, uint64_t *h_plan);
/* The operation over `batch` elements.  h_index: a HOST array of index_width device pointers (plane k: batch * s_k * dL
 * words), h_a: a HOST array of `width` device pointers (plane j: batch * t * dL words, for EACH batch * n * t * dL),
 * h_out: a HOST array of `width` device pointers (output j: batch * t * E_j * dL words).  Planes may alias one another;
 * no output overlaps an input or another output.  CSGN_ERR_INVALID: n_bits 0, an unknown op, index_width outside 1..16,
 * width outside 1..64, rows != 0 for a shift or rotate or outside 1..2^index_width for EACH, `terms` or an s_k of 0 or
 * past the term limit, a null host array, a null device pointer among the first index_width / width entries.
 * CSGN_ERR_UNSUPPORTED: an output of 2^31 words per element or more, or a batch times that (or the source) of 2^60 words
 * or more.  batch == 0 succeeds and touches nothing.  Nothing is allocated or launched before every size is known.  On
 * the caller's stream, asynchronous; the fused form is one launch and graph-capturable.  No GPU: CSGN_ERR_NO_DEVICE, no
 * CPU fallback. */
int csgn_uint_pick(uint64_t n_bits, int op, uint64_t batch, uint64_t index_width, const uint64_t *const *h_index,
                   const uint64_t *h_index_terms, uint64_t width, uint64_t rows, const uint64_t *const *h_a,
                   uint64_t terms, uint64_t *const *h_out, void *stream);

/* EACH over arrays whose ROWS differ in size -- the layout csgn_uint_write (below) leaves, and the sizes of the read that
 * follows it.  Index: index_width = v planes (1..16), plane k uniform with s_k terms.  An array has `rows` = n rows
 * (1 <= n <= 2^v), row r of T[r] >= 1 terms -- the same in every array of the plane --, so an array has A = sum_r T[r]
 * terms and row r begins at term sum_{r' < r} T[r'] of it (a written plane: T[r] = P_r * (tv + td) + td).
 * The read of such a plane by csgn_uint_pick EACH's definition -- element e: the left-nested sum, ascending in r < n, of
 * EQ(x_e, r) * (row r of array e), EQ the LEFT operand -- is UNIFORM: Tout = sum_r P_r * T[r] terms per element,
 * P_r = prod_k (r_k ? s_k : s_k + 1); row r's block begins at term sum_{r' < r} P_{r'} * T[r'], and term in * T[r] + c
 * of the block is (entry in of EQ(x, r), in csgn_uint_read's order) & (term c of the row).  With every T[r] = t these
 * are csgn_uint_pick EACH's words and Tout = t * csgn_uint_pick_terms.  Fresh v = 3, n = 8 over a table written once
 * from one-term planes: T = 17, 9, 9, 5, 9, 5, 5, 3 (A = 62), Tout = 277; in general 2 * 5^v + 3^v.
 * This entry point gives the offsets (host only): h_src_off[r] and h_out_off[r] for r in 0..rows -- rows + 1 entries
 * each -- are row r's first term inside an array and its block's first term inside an output element; entry `rows`
 * holds A and Tout.  CSGN_ERR_INVALID for index_width outside 1..16, rows outside 1..2^index_width, a null pointer, a
 * term count of 0, or a count of 2^62 or more (nothing wraps). */
int csgn_uint_pick_rows_offsets(uint64_t index_width, const uint64_t *h_index_terms, uint64_t rows,
                                const uint64_t *h_row_terms, uint64_t *h_src_off, uint64_t *h_out_off);
/* The read itself is csgn_uint_pick_rows (below).  Its planes may have different rows: h_row_terms holds width * rows
 * counts, plane-major (plane j's T_j[r] at j * rows + r), so plane j has A_j terms per array and Tout_j per output.
 *
 * csgn_uint_pick_rows_check: HOST ONLY, it never touches a device.  Exactly the status csgn_uint_pick_rows returns before
 * it launches anything (that call's first statement is this function's body): CSGN_ERR_INVALID for n_bits 0, index_width
 * outside 1..16, rows outside 1..2^index_width, width outside 1..64, a null pointer, a count of 0, or whatever
 * csgn_uint_pick_rows_offsets refuses for some plane; CSGN_ERR_UNSUPPORTED for a plane with Tout_j * dL of 2^31 words per
 * element or more, or batch * A_j * dL or batch * Tout_j * dL of 2^60 words or more (computed without wrap).  batch == 0 is
 * CSGN_OK.  A test that wants to know whether a size is refused asks here, never the launching call. */
int csgn_uint_pick_rows_check(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *h_index_terms,
                              uint64_t rows, uint64_t width, const uint64_t *h_row_terms);
/* Which form a csgn_uint_pick_rows call of this shape takes (host only, a static string): "k_uint_pick_rows" (one kernel
 * writes every output plane, arrays read in place) or "composed" (per row r: csgn_uint_plain's EQ into a temporary the
 * calling thread keeps (csgn_uint_addk's rules for its composed form), then per plane a pitched copy of the row into a
 * dense temporary and csgn_mul_uniform into the row's block at pitch Tout_j).  Knob "uint_pick_rows_form" (-1 per shape,
 * 0 composed, 1 fused) decides; the words are the same.  Per shape: fused for every shape.  "" where
 * csgn_uint_pick_rows_check refuses the arguments. */
const char *csgn_uint_pick_rows_kernel(uint64_t n_bits, uint64_t batch, uint64_t index_width,
                                       const uint64_t *h_index_terms, uint64_t rows, uint64_t width,
                                       const uint64_t *h_row_terms);
/* h_out[0..2] = (r, in, c) of output position `position` < Tout of ONE plane with the rows h_row_terms[0..rows): the row
 * whose block holds the position, the entry of EQ(x, r) and the term of the row (host only).  It runs the very search of
 * the rows' output offsets and the division by T[r] that the kernel's lanes run, compiled for the host, so the walk can
 * be checked on a CPU.  CSGN_ERR_INVALID for a shape csgn_uint_pick_rows_offsets refuses, a null pointer or a position
 * of Tout or more; CSGN_ERR_UNSUPPORTED where A or Tout reaches 2^32 (the kernel's records are 32-bit; a launch refuses
 * such a plane long before). */
int csgn_uint_pick_rows_decode(uint64_t index_width, const uint64_t *h_index_terms, uint64_t rows,
                               const uint64_t *h_row_terms, uint64_t position, uint64_t *h_out);
/* The calling thread's device memory behind the composed forms, csgn_gather_plan and csgn_uint_pick_rows (host only, it
 * never touches a device): h_out[0] temporary blocks kept, [1] their bytes, [2] blocks retired (handed out under capture,
 * then replaced by growth or eviction; freed at thread exit), [3] hipMalloc calls made for temporaries, [4] hipFree calls
 * made for them (a temporary past 256 MiB is allocated for its call and freed behind it: one of each), [5] row tables
 * kept, [6] row-table device copies retired, [7] row-table device copies freed.  The counts run from the thread's start.
 * CSGN_ERR_INVALID for a null pointer. */
int csgn_scratch_stats(uint64_t h_out[8]);
/* The read over `batch` arrays.  h_index: a HOST array of index_width device pointers (plane k: batch * s_k * dL words),
 * h_arrays: a HOST array of `width` device pointers (plane j: batch * A_j * dL words, csgn_uint_write's output layout),
 * h_out: a HOST array of `width` device pointers (output j: batch * Tout_j * dL words, uniform).  Planes may alias one
 * another; no output overlaps an input or another output.  Statuses: csgn_uint_pick_rows_check's, then CSGN_ERR_INVALID
 * for a null host array or a null device pointer among the first index_width / width entries.  batch == 0 succeeds and
 * touches nothing.  The fused form is one launch.  The calling thread keeps the row tables of the shapes it has used, on
 * the host and on the device (up to 128 tables; planes with equal rows share one): the first call of a shape uploads
 * them and waits for the copy, a repeated call uploads nothing, is asynchronous on the caller's stream and can be
 * captured into a graph (a first call under capture is refused: hipErrorStreamCaptureUnsupported).  A device copy that
 * a capturing stream has used is kept until the thread ends, whatever leaves the cache ("Graphs" at the top).  No GPU:
 * CSGN_ERR_NO_DEVICE, no CPU fallback. */
int csgn_uint_pick_rows(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *const *h_index,
                        const uint64_t *h_index_terms, uint64_t rows, uint64_t width, const uint64_t *const *h_arrays,
                        const uint64_t *h_row_terms, uint64_t *const *h_out, void *stream);

/* ------------------------------------------- encrypted arrays written at encrypted indices ---- */

/* ENCRYPTED arrays written at ENCRYPTED indices: a private counter table, an oblivious register file, one step of an
 * oblivious RAM.  Index: index_width = v planes x_0..x_{v-1} (bit 0 first, v in 1..16) of `batch` elements, plane k
 * uniform with s_k terms per element.  Value: `width` = w planes (1..64) of `batch` elements, plane j uniform with tv_j
 * terms.  Arrays: w planes of batch * n elements (`rows` = n, 1 <= n <= 2^v), plane j uniform with td_j terms; element
 * e's array is the elements e * n .. e * n + n - 1 (csgn_uint_pick's EACH layout).  Output: w planes of batch * n
 * elements.  A fixed composition of the reference's operator+ / operator* with ONE: element e * n + r of plane j is
 *     logicMux(EQ(x_e, r), value_{e,j}, d_{e*n+r,j})  =  (EQ(x_e, r) * (value_{e,j} + d_{e*n+r,j})) + d_{e*n+r,j}
 *     EQ(x, r)   csgn_uint_plain's EQ row with k = r, the LEFT operand of the product, exactly as in csgn_uint_read;
 *                the sum inside is operator+, a concatenation with the value's terms first
 * Decrypts to the arrays with row x_e of array e replaced by value_e, and to the arrays unchanged where x_e >= n.
 * Terms: row r has P_r * (tv_j + td_j) + td_j,  P_r = prod_k R_k(r),  R_k(r) = r_k ? s_k : s_k + 1: the output is
 * RAGGED over r in a pattern of period n (fresh planes: 2^zeros(r) * (tv + td) + td).  Every whole array has
 * A_j = E * (tv_j + td_j) + n * td_j terms, E = csgn_uint_read_terms(v, s, n); row r begins at term
 * csgn_uint_write_offset(v, s, n, r, tv_j, td_j) = csgn_uint_read_terms(v, s, r) * (tv_j + td_j) + r * td_j of its array.
 * Fresh planes: 62 terms per array and plane at v = 3, n = 8; 13 378 at v = 8, n = 256 -- an equality's growth, as for
 * csgn_uint_read.
 * Term order: inside row r, term (q, c) of the product at q * (tv_j + td_j) + c with q the entry of EQ(x, r)
 * (csgn_uint_read's order inside a block) and c < tv_j the value term, else array term c - tv_j; the td_j terms of
 * d_{e*n+r,j} follow. */
/* The term offset of row r inside its array for r in 0..rows (host only); r = rows gives A.  0 for an invalid shape
 * (index_width outside 1..16, rows outside 1..2^index_width, r > rows, a null pointer, a term count of 0) or a count of
 * 2^62 or more -- and for r = 0, where the offset IS 0: test validity with r = rows. */
uint64_t csgn_uint_write_offset(uint64_t index_width, const uint64_t *h_index_terms, uint64_t rows, uint64_t r,
                                uint64_t t_value, uint64_t t_array);
/* Which form a csgn_uint_write call of this shape takes (host only, a static string): "k_uint_write" (one kernel writes
 * every output plane, the rows' raw copies included, planes read in place) or "composed" (per row r: csgn_uint_plain's
 * EQ into a temporary the calling thread keeps (csgn_uint_addk's rules for its composed form), csgn_gather_planes of the
 * elements e * n + r -- the list e * n is uploaded, and waited for, once a call --, then per plane csgn_add_uniform of
 * value and row, csgn_mul_uniform into the row's place and the strided copy of the row behind it).  Knob
 * "uint_write_fused" (-1 per shape, 0 / 1 forced) decides; the words are the same.  Per shape: fused for every shape
 * (batch * n of 2^32 or more is fused whatever the knob says: the gather's counts stop there).  "" for an invalid
 * shape. */
const char *csgn_uint_write_kernel(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *h_index_terms,
                                   uint64_t rows, uint64_t width, const uint64_t *h_value_terms,
                                   const uint64_t *h_array_terms);
/* The fused form's tile for this shape (host only), for tests and tools: h_plan[0..3] = arrays per workgroup, units of a
 * unit slice, E-stream entries a workgroup decodes (QP: workgroup part p owns entries [p * QP, (p + 1) * QP) of the
 * stream of `rows` rows) and the number of such parts.  wide_units: nonzero for the 16-byte-unit kernel (taken when dL
 * is even and every pointer is 16-byte aligned).  CSGN_ERR_INVALID for an invalid shape or an empty batch. */
int csgn_uint_write_plan(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *h_index_terms,
                         uint64_t rows, uint64_t width, const uint64_t *h_value_terms, const uint64_t *h_array_terms,
                         int wide_units, uint64_t *h_plan);
/* The write over `batch` arrays.  h_index: a HOST array of index_width device pointers (plane k: batch * s_k * dL
 * words), h_value: a HOST array of `width` device pointers (plane j: batch * tv_j * dL words), h_arrays: a HOST array of
 * `width` device pointers (plane j: batch * rows * td_j * dL words), h_out: a HOST array of `width` device pointers
 * (output j: batch * A_j * dL words).  Planes may alias one another; no output overlaps an input or another output.
 * CSGN_ERR_INVALID: n_bits 0, index_width outside 1..16, width outside 1..64, rows outside 1..2^index_width, a term
 * count of 0 or past the term limit, a null host array, a null device pointer among the first index_width / width
 * entries.  Limits: every A_j * dL below 2^31 words per array (CSGN_ERR_UNSUPPORTED), batch * that < 2^60.
 * batch == 0 succeeds and touches nothing.  Nothing is allocated or launched before every size is known.  On the
 * caller's stream, asynchronous; the fused form is one launch and graph-capturable.  No GPU: CSGN_ERR_NO_DEVICE, no CPU
 * fallback. */
int csgn_uint_write(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *const *h_index,
                    const uint64_t *h_index_terms, uint64_t rows, uint64_t width, const uint64_t *const *h_value,
                    const uint64_t *h_value_terms, const uint64_t *const *h_arrays, const uint64_t *h_array_terms,
                    uint64_t *const *h_out, void *stream);

/* ------------------------------------------------ encrypted bit matrices over F2 ---- */

/* The product of two ENCRYPTED bit matrices over F2: an inner product of encrypted bit vectors, a secret linear map
 * applied to a batch of encrypted vectors, the parity of every database row with every query.
 * Matrices are uniform CiphertextBatches in row-major order.
 *   - A is rows x inner: element i*inner + e, t_a terms each.
 *   - B is inner x cols: element e*cols + k, t_b terms each.
 *   - In the transposed layout Bt is cols x inner: element k*inner + e.
 *   - C is rows x cols: element i*cols + k, inner * t_a * t_b terms.
 *   - C[i,k] is the left-nested sum, ascending in e, of A[i,e] * B[e,k], with the reference's operator* (left term
 *     slow, right term fast) and operator+ (concatenation).
 *   - Term q of C[i,k] decodes as e = q / (t_a*t_b), a = (q / t_b) % t_a, b = q % t_b.  Its words are
 *     A[i,e][a] & B[e,k][b].
 *   - It decrypts to the matrix product over F2.
 * A sum is a concatenation of term lists, so the product of fresh matrices has `inner` terms per output and adds one
 * level of depth: the growth is the scheme's own. */
/* inner * t_a * t_b (host only); 0 for a zero argument or a count of 2^62 or more. */
uint64_t csgn_matmul_terms(uint64_t inner, uint64_t t_a, uint64_t t_b);
/* Which form a csgn_matmul call of this shape takes (host only, a static string): "k_matmul" (one kernel writes every
 * term of every output element: a workgroup stages a tile's operand terms in LDS once and streams its outputs) or
 * "composed" (both operands tiled to rows * cols * inner elements by csgn_gather's launcher into a temporary the calling
 * thread keeps, under csgn_uint_addk's rules for its composed form, then one csgn_mul_uniform over those pairs straight
 * into the output).  Knob "matmul_form" (-1 per shape, 0 composed, 1 fused) decides; the words are the same.  Per shape:
 * fused.  An operand of 2^32 elements or more is past the gather launcher: such a shape is fused whatever
 * the knob says.  "" for an invalid shape (n_bits 0, a zero dimension, a zero term count or a count of 2^62 or more). */
const char *csgn_matmul_kernel(uint64_t n_bits, uint64_t rows, uint64_t inner, uint64_t cols, uint64_t t_a, uint64_t t_b,
                               int b_transposed);
/* The product.  d_a: rows * inner * t_a * dL words, d_b: inner * cols * t_b * dL words (b_transposed != 0: the layout
 * Bt), d_out: rows * cols * inner * t_a * t_b * dL words.  The operands may alias one another; the output overlaps
 * neither.  Checks, in this order, the first that fails giving the status: n_bits; rows, inner and cols nonzero and
 * t_a, t_b nonzero and below 2^62 (CSGN_ERR_INVALID); inner * t_a * t_b * dL below 2^31 words per element and the
 * output below 2^60 words (CSGN_ERR_UNSUPPORTED; computed without wrap-around); null device pointers
 * (CSGN_ERR_INVALID); the device (CSGN_ERR_NO_DEVICE, no CPU fallback).  Nothing is allocated or launched before every
 * check has passed.  On the caller's stream, asynchronous; the fused form is one launch for every shape within memory
 * and graph-capturable. */
int csgn_matmul(uint64_t n_bits, uint64_t rows, uint64_t inner, uint64_t cols, const uint64_t *d_a, uint64_t t_a,
                const uint64_t *d_b, uint64_t t_b, int b_transposed, uint64_t *d_out, void *stream);

/* ------------------------------------------------ encrypted bits counted into integers ---- */

/* ENCRYPTED bits counted into ENCRYPTED integers: COUNT(*) of matching rows, the Hamming weight of a word, the Hamming
 * distance of two words.  Bit j of the number of ones among g bits is the elementary symmetric polynomial of degree
 * 2^j over F2 (Lucas).
 * Inputs: g ciphertexts x_0 ... x_{g-1} per output element, each of t terms.
 * For a plane index j with m = 2^j <= g, output plane j of element q is the left-nested sum (operator+, a
 * concatenation) of the left-nested products x_{i_1} * x_{i_2} * ... * x_{i_m}.  In each product the left term is slow
 * and the right term fast, as in the reference's operator*.  The sum runs over the m-subsets i_1 < i_2 < ... < i_m of
 * {0 ... g-1} in LEXICOGRAPHIC ORDER.  This is the order of the nested loops `for i_1 < i_2 < ...`.
 *   - Plane j has T_j = C(g, m) * t^m terms.
 *   - Term p decodes as c = p / t^m and digits d_1 ... d_m of p mod t^m in base t, with d_1 slowest.  Its words are the
 *     AND over k of term d_k of x_{i_k}, where (i_1 ... i_m) is the subset of lexicographic rank c.
 *   - Plane j decrypts to bit j of the number of ones.
 *   - Plane 0 is the concatenation of the inputs: what sumGroups(g) already returns without a launch.
 *   - With 2^j > g the bit is always 0.  The C ABI refuses such a j.  The classes return the one-term ZERO of
 *     constantBatch.
 * Term counts of the definition: g = 64, t = 1: planes 0, 1, 2 have 64, 2016 and 635 376 terms; planes 3, 4, 5 of
 * g = 64 are past any memory; plane 6 of g = 64 is one term, the AND of all 64; g = 65: plane 6 has 65 terms.  Because
 * of this, a call names the planes it wants as a list.  It does not give a range. */
/* C(group, 2^j) * t^(2^j) (host only); 0 for a zero argument, j > 6, 2^j > group, t >= 2^62 or a count of 2^62 or more */
uint64_t csgn_count_terms(uint64_t group, uint64_t t, uint64_t j);
/* "k_count", "composed", or "" for an invalid shape (host only, a static string).  "k_count": one kernel writes every
 * requested plane of every element; a workgroup stages its element's input terms in LDS once, unranks the subsets of
 * its range of ranks and streams its outputs.  "composed": per plane, the m index lists of the count * C(g, m) pairs
 * (element, subset), every factor tiled to the pairs by csgn_gather's launcher into a temporary the calling thread
 * keeps (csgn_uint_addk's rules for its composed form), and m - 1 csgn_mul_uniform, the last straight into the output;
 * the plane layout is interleaved into one grouped batch first.  Knob "count_form" (-1 per shape, 0 composed, 1 fused)
 * decides; the words are the same.  Per shape: fused.  A call of count * group >= 2^32 inputs is past the
 * gather launcher: such a shape is fused whatever the knob says.  Invalid: n_bits 0, the arguments csgn_count refuses
 * with CSGN_ERR_INVALID, or a plane of 2^62 terms or more. */
const char *csgn_count_kernel(uint64_t n_bits, uint64_t count, uint64_t group, uint64_t t, uint64_t n_in,
                              uint64_t n_out, const uint64_t *h_js);
/* The count over `count` elements.  h_in: a HOST array of n_in device pointers.  n_in == 1, the grouped layout: one
 * batch of count * group elements, input i of element q is element q * group + i.  n_in == group with 2 <= group <= 64,
 * the plane layout: input i is a batch of `count` elements (what a UIntBatch hands over).  h_js: n_out strictly
 * ascending plane indices; h_out[x] takes count * T_{h_js[x]} * dL words.  Inputs may alias one another; no output
 * overlaps an input or another output.  Checks, in this order, the first that fails giving the status: n_bits; count,
 * group, t nonzero, t < 2^62, n_in 1 or group (<= 64 when above 1), n_out >= 1, the js strictly ascending with
 * 2^j <= group, host pointers non-null (CSGN_ERR_INVALID); every T_j * dL below 2^31 words per element and
 * count * T_j * dL below 2^60 (CSGN_ERR_UNSUPPORTED; computed without wrap-around); null device pointers
 * (CSGN_ERR_INVALID); the device (CSGN_ERR_NO_DEVICE, no CPU fallback).  Nothing is allocated or launched before every
 * check has passed.  On the caller's stream, asynchronous; the fused form is one launch for every shape within memory
 * and graph-capturable. */
int csgn_count(uint64_t n_bits, uint64_t count, uint64_t group, uint64_t t, const uint64_t *const *h_in, uint64_t n_in,
               uint64_t n_out, const uint64_t *h_js, uint64_t *const *h_out, void *stream);

/* RUNNING counts of encrypted bits: for every row r of a group, how many of the rows up to and including r (exclusive
 * = 0) or before r (exclusive = 1) have their bit set -- a cumulative count, the rank of a row among the matching rows,
 * the segment number of a row, the rank function of a bit vector, a running parity (plane 0).
 * Inputs: csgn_count's, g = group inputs x_0 ... x_{g-1} of t terms per element, in either layout.  Row r, 0 <= r < g,
 * counts the inputs x_0 ... x_{n_r - 1}, n_r = r + 1 - exclusive.  For a plane j with m = 2^j:
 *   - m <= n_r: output (r, j) of element q is WORD FOR WORD csgn_count's plane j of those n_r inputs: the m-subsets of
 *     {0 ... n_r - 1} in lexicographic order, term p = rank * t^m + digits (d_1 slowest), the AND of the factors' terms;
 *     T_{r,j} = C(n_r, m) * t^m terms.
 *   - m > n_r (n_r = 0 among them): the one all-zero term, the ZERO of constantBatch; T_{r,j} = 1.
 * Layout, by row: h_out[x] is one block for plane j = h_js[x]; in it row r is a uniform batch of `count` elements of
 * T_{r,j} terms each that begins at term count * off_j(r), off_j(r) the sum of T_{r',j} over r' < r:
 *   inclusive off_j(r) = min(r, m - 1) + C(r + 1, m + 1) * t^m,  exclusive off_j(r) = min(r, m) + C(r, m + 1) * t^m.
 * A_j = off_j(g); the block takes count * A_j * dL words.  Every row is a uniform batch every other entry point takes;
 * with even dL every row begins on a 16-byte boundary whenever the block does.
 * Term counts: fresh flags, g = 16: A_j = 136, 681, 6191, 24 317 and 16 for planes 0 to 4; g = 64: 2080 and 43 681 for
 * planes 0 and 1. */
/* off_j(r), r in 0..group, r = group giving A_j (host only).  0 for an invalid shape (a zero argument, exclusive above
 * 1, j > 6, 2^j > group - exclusive, t >= 2^62, r > group) or a value of 2^62 or more -- and for r = 0, whose offset IS
 * 0: test a shape's validity with r = group. */
uint64_t csgn_count_prefix_offset(uint64_t group, uint64_t t, uint64_t j, uint64_t exclusive, uint64_t r);
/* The running counts of `count` elements in one kernel, k_count_prefix.  h_in, n_in: as in csgn_count.  h_js: n_out
 * strictly ascending plane indices with 2^j <= group - exclusive (a higher plane is ZERO in every row: the classes
 * return it without a launch).  Inputs may alias one another; no output overlaps an input or another output.  Checks,
 * in this order, the first that fails giving the status: n_bits; count, group, t nonzero, t < 2^62, exclusive 0 or 1,
 * n_in 1 or group (<= 64 when above 1), n_out >= 1, host pointers non-null, the js strictly ascending with 2^j <=
 * group - exclusive (CSGN_ERR_INVALID); every T_{r,j} * dL below 2^31 words and count * A_j * dL below 2^60
 * (CSGN_ERR_UNSUPPORTED; computed without wrap-around); null device pointers (CSGN_ERR_INVALID); the device
 * (CSGN_ERR_NO_DEVICE, no CPU fallback).  Nothing is allocated or launched before every check has passed.  On the
 * caller's stream, asynchronous; one launch for every shape within memory (the ZERO terms of the short rows are
 * written by it too) and graph-capturable.  Knob "count_cpart" places the split of the ranks over workgroups as it does
 * for k_count. */
int csgn_count_prefix(uint64_t n_bits, uint64_t count, uint64_t group, uint64_t t, uint64_t exclusive,
                      const uint64_t *const *h_in, uint64_t n_in, uint64_t n_out, const uint64_t *h_js,
                      uint64_t *const *h_out, void *stream);

/* ------------------------------------------------ encrypted integers summed into integers ---- */

/* ENCRYPTED integers summed into ENCRYPTED integers: SUM(value) of the matching rows, the product of two encrypted
 * integers, the inner product of two vectors of them.  For bits x_i of public weights 2^{e_i}, bit j of
 * S = sum 2^{e_i} x_i is C(S, 2^j) mod 2, the coefficient of z^(2^j) in (1 + z)^S; over F2,
 * (1 + z)^(2^e x) = 1 + x z^(2^e).  So bit j of S is the sum, over the subsets of inputs whose weights add up to
 * EXACTLY 2^j, of the product of their members.  With all weights 1 this is csgn_count's definition.
 * Inputs.  An output element has C weight classes, 1 <= C <= 64.
 *   - Class c holds n_c >= 0 ciphertexts of weight 2^c, each of t terms.
 *   - t is uniform over the call.
 *   - sum n_c >= 1 and sum n_c <= 65 536.
 * Output plane j (j <= 62) of element q is the left-nested sum (operator+, a concatenation) of monomials, in this
 * order:
 *   1. Count vectors.  A count vector is (m_j, m_{j-1}, ..., m_0) with sum m_c 2^c = 2^j and 0 <= m_c <= n_c.  Take
 *      n_c = 0 for c >= C.  Classes above j never take part.
 *      - The vectors come in ascending lexicographic order, m_j most significant.
 *      - This is the order of the nested loops `for m_j = 0...: for m_{j-1} = 0...: ...`, with m_0 the remainder,
 *        skipped when it exceeds n_0.
 *   2. Selections within a vector.  A selection is (S_j, ..., S_0), S_c an m_c-subset of class c.  S_j is slowest and
 *      S_0 fastest.  Each class's subsets run in lexicographic order (csgn_count's order).
 *   3. The monomial of a selection.  It is the left-nested product (operator*, left term slow) of its members:
 *      classes descending, indices ascending within a class.  It has t^(sum m_c) terms, the first factor's digit
 *      slowest.
 * Term count.  T_j = sum over the vectors of prod_c C(n_c, m_c) t^{m_c}.
 *   - With one class, plane j has exactly csgn_count's words.
 *   - A plane with no count vector is always 0.  The C ABI refuses it.  The classes return the one-term ZERO.
 * Term counts of fresh inputs (t = 1), planes 0, 1, 2, ...: the sum of 4 three-bit integers 4, 10, 35, 161, 315; of 8
 * four-bit integers 8, 36, 330, 6435, 245 149; a 4 x 4 -> 8 bit product 1, 2, 4, 10, 34, 129, 383, 511; the low 8 bits of
 * an 8 x 8 product 1, 2, 4, 10, 36, 202, 1828, 27 338.  The higher planes of wide groups are past any memory: a call
 * names the planes it wants as a list. */
/* T_j (host only).  h_n: n_classes counts.  0 for a bad argument (n_classes outside 1..64, a null h_n, sum n_c outside
 * 1..65 536, t = 0 or t >= 2^62, j > 62), for a plane with no count vector, or for a count of 2^62 or more. */
uint64_t csgn_wsum_terms(uint64_t n_classes, const uint64_t *h_n, uint64_t t, uint64_t j);
/* A plan: the count vectors of the planes h_js (n_out of them, 1..63, strictly ascending) of one shape (n_c, t),
 * enumerated with pruning and uploaded once, synchronously: per plane and vector the first term, the selections, every
 * m_c, C(n_c, m_c) and the degree.  Checks, in this order: plan non-null, the arguments csgn_wsum_terms refuses, n_out,
 * h_js, a plane with no count vector (CSGN_ERR_INVALID); a plane of 2^31 terms or more (CSGN_ERR_UNSUPPORTED); the
 * device (CSGN_ERR_NO_DEVICE); then, while enumerating, more than 65 536 vectors over the planes, or a monomial of more
 * than 3072 factors (CSGN_ERR_UNSUPPORTED).  Knob "wsum_cpart" is read here: it forces the selection ranks of a
 * workgroup's part. */
typedef struct csgn_wsum_plan csgn_wsum_plan;
int csgn_wsum_create(uint64_t n_classes, const uint64_t *h_n, uint64_t t, uint64_t n_out, const uint64_t *h_js,
                     csgn_wsum_plan **plan);
/* T of the plan's plane x (host only); 0 for a null plan or x past its planes */
uint64_t csgn_wsum_plan_terms(const csgn_wsum_plan *plan, uint64_t x);
void csgn_wsum_destroy(csgn_wsum_plan *plan);
/* The sum over `count` elements in one kernel, k_wsum: a workgroup stages the inputs of the classes that take part in
 * LDS once, unranks the selections of its part of one count vector and streams its outputs.  h_in: a HOST array of C
 * device pointers.  Class c is one batch of count * n_c elements; input i of element q is element q * n_c + i.  The
 * pointer may be null where n_c = 0.  h_out[x] takes count * T_{js[x]} * dL words.  Inputs may alias one another; no
 * output overlaps an input or another output.  Checks, in this order, the first that fails giving the status: n_bits;
 * plan, count nonzero, host pointers non-null (CSGN_ERR_INVALID); every T_j * dL below 2^31 words per element and
 * count * T_j * dL and every class's count * n_c * t * dL below 2^60 (CSGN_ERR_UNSUPPORTED; computed without
 * wrap-around); null device pointers (CSGN_ERR_INVALID); the device (CSGN_ERR_NO_DEVICE, no CPU fallback).  Nothing is
 * allocated or launched before every check has passed.  On the caller's stream, asynchronous; one launch for every
 * shape within memory and graph-capturable. */
int csgn_wsum(const csgn_wsum_plan *plan, uint64_t n_bits, uint64_t count, const uint64_t *const *h_in,
              uint64_t *const *h_out, void *stream);

/* ------------------------------------------------------------------- tuning ---- */

/* Kernel-choice and sweep knobs ("mul_flat", "mul_touch", "ragged_c", "perm_ballot", ...;
 * csgn_tuning_name(i) enumerates them, NULL past the end; csgn_amd/csrc/csgn_tuning.h documents
 * each).  A knob's start value is its built-in default or the environment variable
 * CSGN_<KEY IN CAPITALS>, sampled ONCE when the library is loaded: no compute entry point reads
 * the environment.  Knobs choose among kernels that produce the same words; results never depend
 * on them.  They are PER HOST THREAD: csgn_set_tuning changes the dispatch of the calling thread's own
 * later calls and of no other thread's (every thread starts from the defaults + the environment
 * snapshot), so concurrent one-thread-per-GPU callers cannot switch one another's kernels.
 * A circuit (csgn_circuit_build) bakes in the building thread's values at build time. */
/* Sharing the GPU.  The default dispatch of a large all-pairs multiply (operand touch pass + flat
 * kernel) is tuned for a caller that has the chip to itself: measured 7.3 TB/s alone, but 3.5 TB/s
 * beside a second stream of back-to-back 1 GiB device copies, where the LDS-tiled kernel holds 4.8
 * (6.9 alone; profiles/r03/cotenant_ab.json).  A host thread whose GPU also serves other streams or
 * processes should call csgn_set_tuning("shared_gpu", 1) (or start with CSGN_SHARED_GPU=1 in the
 * environment): its multiplies then take the kernel that does not depend on what the memory-side
 * cache holds.  Results are identical either way. */
int csgn_set_tuning(const char *key, int value);
int csgn_get_tuning(const char *key, int *h_value);
void csgn_reset_tuning(void);            /* defaults + the environment snapshot taken at load */
const char *csgn_tuning_name(int index);

/* Debug hook: quotient n/d computed by the same division-by-invariant helper the kernels
 * use (csgn_amd/csrc/csgn_common.h); lets the CPU tests pin it without a GPU. */
uint32_t csgn_debug_fastdiv(uint32_t n, uint32_t d);

/* Debug hook: the logical index that workgroup b of a launch of nblocks workgroups takes under the XCD block orders
 * the kernels use (csgn_amd/csrc/csgn_device.h): group = 0 is xcd_contiguous_block, group > 0 xcd_grouped_block. */
uint32_t csgn_debug_block_order(uint32_t b, uint32_t nblocks, uint32_t group);

#ifdef __cplusplus
}
#endif
#endif
