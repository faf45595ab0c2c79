// csgn_uint_decrypt.hip -- up to 64 one-bit batches decrypted into ONE word per element in one pass (csgn_uint_decrypt,
// include/csgn_hip.h): bit j of values[e] = Dec(element e of plane j) = XOR over the element's terms of (the term covers
// the key mask).  Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in DESIGN.md §4.29.
//
// Work decomposition (all of it in closed form from the batch and the term counts; nothing is planned on the device):
//   - A workgroup OWNS 4 * GW consecutive elements for ALL planes, a wave GW of them.  The terms of a wave's elements in
//     one plane are one contiguous stream of whole terms (uniform: elements * T_j terms; ragged: off[first] .. off[last]),
//     which the wave reads with 16-byte (8-byte) units, lane after lane, kPasses loads of a lane in flight.  Every pass
//     ballots "my unit covers the mask"; the lane that holds a term's LAST unit tests the term's bits of the ballot (a
//     term that began in an earlier pass carries one wave-uniform flag over), and a hit flips bit j of the element's word
//     in LDS.  After the last plane the words leave with plain stores: no hit bitmap, no partial parity and no atomic
//     reaches HBM.
//   - Only an element of a UNIFORM plane with more than `chunk` terms is cut: every chunk of `chunk` terms is an item a
//     wave of the workgroups behind the owning ones takes; it folds its hits into one parity and XORs one bit into the
//     value word with a 64-bit vector atomic.  In that form, and only in it, the words are zeroed first (zero_words) and
//     the owning workgroups XOR their words in too.
// The launch is split only at launch_blocks() workgroups.
#include "csgn_device.h"

namespace csgn {

namespace {

constexpr u32 kPasses = 4;                    // loads a lane keeps in flight
constexpr u32 kMaxGW = kWave;                 // elements a wave owns at most: the workgroup's words are 256
constexpr u32 kChunkByShape = 1024;           // knob uint_decrypt_chunk = 0
constexpr u64 kFillBlocks = 2048;             // owning workgroups wanted before GW stops shrinking: eight a CU
constexpr u64 kMinBlockTerms = 256;           // ... unless a workgroup would hold fewer terms than this

// by value in the kernel arguments
struct DecryptArgs {
    const void *plane[kUintDecryptMaxPlanes];
    const u64 *off[kUintDecryptMaxPlanes];    // a ragged plane's CSR offsets, nullptr: uniform
    u32 terms[kUintDecryptMaxPlanes];         // uniform: terms per element; ragged: the bound on one element's terms
    FastDivTable<kUintDecryptMaxPlanes> dT;   // terms[j] of the uniform planes as divisors
    const void *mask;
    u64 *values;
    u64 batch;
    u64 block0;                               // the first logical workgroup of this launch
    u64 owned_blocks;                         // logical workgroups [0, owned_blocks) own elements, the rest take items
    u64 items, items_per_elem;                // chunks of the cut planes: all of them, and of one element
    u32 n_planes, U, GW, chunk;
    FastDiv dU;
};
static_assert(sizeof(DecryptArgs) <= 4096, "the kernel arguments of k_uint_decrypt pass the 4 KiB limit");

// One pass of a wave over 64 consecutive units of a stream of U-unit terms; b = the ballot of "unit covers the mask".
// The verdict of the lane that holds the LAST unit of a term: every unit of the term covers the mask.  open_ok: the
// same over the units an earlier pass held of the term that was open at this pass's first unit.
__host__ __device__ inline bool term_verdict(u64 b, u32 lane, u32 U, bool open_ok)
{
    if (lane + 1u >= U) {                                        // the term began in this pass, at lane + 1 - U
        const u64 m = (U >= 64u ? ~0ull : (1ull << U) - 1ull) << (lane + 1u - U);
        return (b & m) == m;
    }
    const u64 m = ~0ull >> (63u - lane);                         // bits 0 .. lane
    return open_ok && (b & m) == m;
}

// open_ok for the next pass: `start` = the first unit of the term that holds unit pass0 + 64 (the next pass's first)
__host__ __device__ inline bool term_open(u64 b, u32 pass0, u32 start, bool open_ok)
{
    if (start == pass0 + 64u)                                    // the next pass begins a term
        return true;
    if (start >= pass0) {
        const u32 l0 = start - pass0;
        return (b >> l0) == (~0ull >> l0);
    }
    return open_ok && b == ~0ull;
}

// A wave streams the nu units of nu / U whole terms from `base` and calls f(hit, t) once a pass, in every lane: hit = the
// lane holds the last unit of term t (counted from base) and the term covers the mask.  Loads are unconditional
// (clamped into the stream) so that kPasses of them are in flight (csgn_decrypt.hip, k_term_hits_seg).  Every lane of
// the wave must call it, with wave-uniform arguments but `lane`.
template <typename Unit, typename F>
__device__ inline void wave_term_hits(const Unit *__restrict__ base, u32 nu, u32 U, const FastDiv &dU,
                                      const Unit *__restrict__ mask, u32 lane, F f)
{
    bool open_ok = true;
    const u32 last = nu - 1u;
    for (u32 g0 = 0; g0 < nu; g0 += kWave * kPasses) {
        Unit x[kPasses], mk[kPasses];
        u32 t[kPasses], k[kPasses];
#pragma unroll
        for (u32 j = 0; j < kPasses; ++j) {
            const u32 g = g0 + j * kWave + lane;
            x[j] = base[g < last ? g : last];
        }
#pragma unroll
        for (u32 j = 0; j < kPasses; ++j) {
            const u32 g = g0 + j * kWave + lane;
            t[j] = csgn_fastdiv(g, dU);
            k[j] = g - t[j] * U;
            mk[j] = mask[k[j]];
        }
#pragma unroll
        for (u32 j = 0; j < kPasses; ++j) {
            const u32 pass0 = g0 + j * kWave, g = pass0 + lane;
            if (pass0 >= nu)
                break;
            const u64 b = __ballot(g < nu && unit_covers(x[j], mk[j]));
            const bool hit = g < nu && k[j] == U - 1u && term_verdict(b, lane, U, open_ok);
            f(hit, t[j]);
            open_ok = term_open(b, pass0, csgn_fastdiv(pass0 + kWave, dU) * U, open_ok);
        }
    }
}

template <typename Unit, bool CUT>
__global__ void __launch_bounds__(256) k_uint_decrypt(DecryptArgs a)
{
    __shared__ u64 vals[4 * kMaxGW];                             // the workgroup's value words
    __shared__ u64 offs[4][kMaxGW + 1];                          // a wave's offsets in the ragged plane at hand
    const u32 tid = threadIdx.x, lane = tid & (kWave - 1);
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const u64 bid = a.block0 + blockIdx.x;
    const Unit *mask = reinterpret_cast<const Unit *>(a.mask);
    const u32 U = a.U;

    if (CUT && bid >= a.owned_blocks) {
        // item = (element, chunk of a cut plane): one wave folds the chunk's hits and XORs one bit into the word
        const u64 item = (bid - a.owned_blocks) * 4u + wave;
        if (item >= a.items)
            return;
        const u64 e = item / a.items_per_elem;
        u64 q = item - e * a.items_per_elem;
        u32 j = 0, T = 0;
        for (; j < a.n_planes; ++j) {
            T = a.terms[j];
            if (a.off[j] || T <= a.chunk)
                continue;
            const u32 nch = (T + a.chunk - 1u) / a.chunk;
            if (q < nch)
                break;
            q -= nch;
        }
        if (j >= a.n_planes)
            return;                                              // (never: items_per_elem is the sum of the nch)
        const u32 t0 = (u32)q * a.chunk, nt = min(a.chunk, T - t0);
        const Unit *base = reinterpret_cast<const Unit *>(a.plane[j]) + (e * T + t0) * U;
        u32 par = 0;
        wave_term_hits(base, nt * U, U, a.dU, mask, lane, [&](bool hit, u32) { par ^= (u32)__popcll(__ballot(hit)); });
        if (lane == 0 && (par & 1u))
            atomicXor(reinterpret_cast<unsigned long long *>(a.values + e), 1ull << j);
        return;
    }

    vals[tid] = 0ull;
    __syncthreads();
    const u32 GW = a.GW;
    const u64 e0 = bid * (4u * GW), ea = e0 + (u64)wave * GW;    // the workgroup's and the wave's first element
    const u32 ne = ea < a.batch ? (u32)min((u64)GW, a.batch - ea) : 0u;
    u64 *mine = vals + wave * GW;
    for (u32 j = 0; j < a.n_planes; ++j) {
        const u64 *off = a.off[j];
        const u32 T = a.terms[j];
        const u64 bit = 1ull << j;
        const Unit *plane = reinterpret_cast<const Unit *>(a.plane[j]);
        if (off) {                                               // ragged (the same branch in all four waves)
            __syncthreads();                                     // the plane before is done with offs
            if (ne)
                for (u32 i = lane; i <= ne; i += kWave)
                    offs[wave][i] = off[ea + i];
            __syncthreads();
            if (ne == 0)
                continue;
            const u64 *wo = offs[wave];
            const u64 s0 = wo[0];
            // (a bound that does not hold is the caller's error; it still never makes the stream longer than stated)
            const u32 nt = (u32)min(wo[ne] - s0, (u64)ne * T);
            if (nt == 0)
                continue;
            wave_term_hits(plane + s0 * U, nt * U, U, a.dU, mask, lane, [&](bool hit, u32 t) {
                if (hit) {
                    const u64 at = s0 + t;                       // the last element whose offset is at or before it
                    u32 lo = 0, hi = ne;
                    while (hi - lo > 1u) {
                        const u32 mid = lo + ((hi - lo) >> 1);
                        if (wo[mid] <= at)
                            lo = mid;
                        else
                            hi = mid;
                    }
                    atomicXor(reinterpret_cast<unsigned long long *>(mine + lo), bit);
                }
            });
        } else if (ne && !(CUT && T > a.chunk)) {
            const FastDiv dT = a.dT.at(j);
            wave_term_hits(plane + ea * T * U, ne * T * U, U, a.dU, mask, lane, [&](bool hit, u32 t) {
                if (hit)
                    atomicXor(reinterpret_cast<unsigned long long *>(mine + csgn_fastdiv(t, dT)), bit);
            });
        }
    }
    __syncthreads();
    const u64 e = e0 + tid;
    if (tid < 4u * GW && e < a.batch) {
        if (!CUT)
            a.values[e] = vals[tid];
        else if (vals[tid])
            atomicXor(reinterpret_cast<unsigned long long *>(a.values + e), vals[tid]);
    }
}

// terms of one element and plane a wave takes before the element is cut
u32 decrypt_chunk()
{
    const int forced = tune(TUNE_UINT_DECRYPT_CHUNK);
    return forced > 0 ? (u32)std::min<u64>((u64)forced, kLongTerms) : kChunkByShape;
}

bool decrypt_shape_ok(u64 n_bits, u64 batch, u64 n_planes, const u64 *terms)
{
    return n_bits != 0 && batch != 0 && n_planes >= 1 && n_planes <= kUintDecryptMaxPlanes && terms != nullptr;
}

template <typename Unit, bool CUT>
hipError_t decrypt_launch(DecryptArgs &a, u64 total_blocks, hipStream_t st)
{
    const u64 max_blocks = launch_blocks();
    for (u64 b0 = 0; b0 < total_blocks; b0 += max_blocks) {
        a.block0 = b0;
        k_uint_decrypt<Unit, CUT><<<(u32)std::min(max_blocks, total_blocks - b0), 256, 0, st>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace

// ------------------------------------------------------------------------------ public

const char *uint_decrypt_kernel_name(u64 n_bits, u64 batch, u64 n_planes, const u64 *terms)
{
    if (!decrypt_shape_ok(n_bits, batch, n_planes, terms))
        return "";
    const u32 chunk = decrypt_chunk();
    for (u64 j = 0; j < n_planes; ++j)
        if (terms[j] > chunk)
            return "k_zero_words+k_uint_decrypt";
    return "k_uint_decrypt";
}

hipError_t uint_decrypt(u64 n_bits, u64 batch, u64 n_planes, const u64 *const *planes, const u64 *terms,
                        const u64 *const *off, const u64 *max_terms, const u64 *mask, u64 *values, hipStream_t stream)
{
    if (!decrypt_shape_ok(n_bits, batch, n_planes, terms))
        return hipErrorInvalidValue;
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(planes, n_planes), mask);
    DecryptArgs a = {};
    a.mask = mask;
    a.values = values;
    a.batch = batch;
    a.n_planes = (u32)n_planes;
    a.U = (u32)(wide ? dL / 2 : dL);
    a.dU = csgn_fastdiv_make(a.U);
    a.chunk = decrypt_chunk();
    // the terms of one element in the planes its workgroup owns (a ragged plane: its bound), and its items
    u64 own_terms = 0;
    for (u64 j = 0; j < n_planes; ++j) {
        const bool ragged = terms[j] == 0;
        if (ragged && (!off || !off[j] || !max_terms || max_terms[j] > kLongTerms))
            return hipErrorInvalidValue;
        const u64 T = ragged ? max_terms[j] : terms[j];
        if (T >= (1ull << 31))
            return hipErrorInvalidValue;
        a.plane[j] = planes[j];
        a.off[j] = ragged ? off[j] : nullptr;
        a.terms[j] = (u32)T;
        a.dT.set((u32)j, (u32)std::max<u64>(T, 1));
        if (!ragged && T > a.chunk)
            a.items_per_elem += (T + a.chunk - 1) / a.chunk;
        else
            own_terms += T;
    }
    if (a.items_per_elem && !term_mul(batch, a.items_per_elem, a.items))
        return hipErrorInvalidValue;
    // GW: as many elements a wave as its words allow, fewer while the owning workgroups would not fill the chip and a
    // workgroup still holds kMinBlockTerms terms
    u32 GW = kMaxGW;
    while (GW > 1 && (batch + 4 * GW - 1) / (4 * GW) < kFillBlocks && 2 * GW * own_terms >= kMinBlockTerms)
        GW /= 2;
    a.GW = GW;
    // (every plane cut: the zero fill has written the words, nothing is owned)
    a.owned_blocks = own_terms || !a.items_per_elem ? (batch + 4 * GW - 1) / (4 * GW) : 0;
    const u64 total_blocks = a.owned_blocks + (a.items + 3) / 4;
    if (a.items_per_elem == 0)
        return wide ? decrypt_launch<unit16, false>(a, total_blocks, stream)
                    : decrypt_launch<unit8, false>(a, total_blocks, stream);
    const hipError_t e = zero_words(values, batch, stream);
    if (e != hipSuccess)
        return e;
    return wide ? decrypt_launch<unit16, true>(a, total_blocks, stream)
                : decrypt_launch<unit8, true>(a, total_blocks, stream);
}

} // namespace csgn
