// csgn_matmul.hip -- the product of two ENCRYPTED bit matrices over F2, every term of every output element in one
// launch.  Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in DESIGN.md §4.20.
//
// The definition (include/csgn_hip.h, csgn_matmul): C[i,k] is the left-nested sum, ascending in e, of A[i,e] * B[e,k];
// a sum is a concatenation, so term q of C[i,k] is A[i,e][a] & B[e,k][b] with e = q / (t_a t_b), a = (q / t_b) % t_a,
// b = q % t_b.  Every A[i,e] term is used `cols` times and every B[e,k] term `rows` times.
//
// A workgroup owns a tile of RT rows by CT columns of C, a range of EP values of e and a slice of KC units of every
// term.  It stages its RT * EP left elements and CT * EP right elements in LDS once (each read from memory once per
// tile instead of once per output) and then walks the stream of its outputs with the unit fastest, then b, a, e and
// the output element, so one store instruction writes 64 consecutive units of one output element.  When rows * cols
// alone cannot fill the chip (an inner product, a thin matrix-vector product) the range of e is cut over workgroups;
// every part writes its own slice of the output stream, so nothing is accumulated and no atomics are needed.  A 1 x 1
// tile has no reuse to offer and reads its operands straight from memory (Staged = false), as does a shape whose
// terms do not fit the LDS budget.
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u64 kLdsBudget = 32768;       // bytes of staged operands per workgroup: five workgroups (20 waves) a CU
constexpr u32 kMaxTile = 8;             // rows, and columns, of a tile at most: each staged term is used 8 times
constexpr u32 kMinChunk = 16;           // units of a term slice at least, when terms are cut to fit the LDS
constexpr u64 kTargetUnits = 16384;     // units a workgroup writes at most by choice (256 KiB of 16-byte units)
constexpr u64 kMinUnits = 2048;         // ... and at least, when the range of e is cut further to fill the chip
constexpr u64 kFillBlocks = 2048;       // workgroups that fill 256 CUs (eight resident each)
constexpr u64 kMaxStream = 0xFFFFFE00ull;  // units of one workgroup's stream at most: its 32-bit index never wraps

// By value in the kernel arguments (uniform, scalar loads).  A workgroup is (row tile, column tile, e part, unit
// chunk), the chunk fastest.  Rows and columns are those of this launch (row0 / col0: its first ones in the call).
struct MatmulArgs {
    const void *A, *B;
    void *C;
    u64 inner, cols;            // of the whole call
    u64 b_se, b_sk;             // B's element index = e * b_se + k * b_sk (transposed: 1 and inner)
    u64 row0, col0;
    u32 nrows, ncols;           // of this launch
    u32 ta, tb, U, KC, RT, CT, EP, chunks, eparts, ctiles, nblocks, xcd;
    u32 abase;                  // byte offset of the right operand's terms in the LDS
    FastDiv dKC, dTA, dTB, dTTKC, dEP, dCT;
};

// `outer` x EP elements of t terms, units [k0, k0 + kc) of every term, into lds[((o * EP + ee) * t + c) * KC + kk];
// element (o, ee) of the source is element (o0 + o) * s_o + (e0 + ee) * s_e
template <typename Unit>
__device__ inline void stage(Unit *lds, const Unit *__restrict__ src, u32 outer, u32 n_outer, u64 o0, u64 s_o, u64 e0,
                             u64 s_e, u32 ne, const MatmulArgs &a, u32 t, const FastDiv &dT, u32 k0, u32 kc)
{
    const u32 n = outer * a.EP * t * a.KC;
    for (u32 x = threadIdx.x; x < n; x += 256u) {
        const u32 m = csgn_fastdiv(x, a.dKC), kk = x - m * a.KC;
        const u32 oe = csgn_fastdiv(m, dT), c = m - oe * t;
        const u32 o = csgn_fastdiv(oe, a.dEP), ee = oe - o * a.EP;
        if (o >= n_outer || ee >= ne || kk >= kc)
            continue;
        lds[x] = src[(((o0 + o) * s_o + (e0 + ee) * s_e) * t + c) * a.U + k0 + kk];
    }
}

template <typename Unit, bool Staged>
__global__ void __launch_bounds__(256) k_matmul(MatmulArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    Unit *As = reinterpret_cast<Unit *>(smem_raw);
    Unit *Bs = reinterpret_cast<Unit *>(smem_raw + a.abase);
    const Unit *__restrict__ A = reinterpret_cast<const Unit *>(a.A);
    const Unit *__restrict__ B = reinterpret_cast<const Unit *>(a.B);
    Unit *__restrict__ C = reinterpret_cast<Unit *>(a.C);
    const u32 bid = a.xcd ? xcd_contiguous_block(blockIdx.x, a.nblocks) : blockIdx.x;
    const u32 te = bid / a.chunks, chunk = bid - te * a.chunks;
    const u32 tile = te / a.eparts, epart = te - tile * a.eparts;
    const u32 tr = tile / a.ctiles, tc = tile - tr * a.ctiles;
    const u32 r0 = tr * a.RT, nr = min(a.RT, a.nrows - r0);
    const u32 c0 = tc * a.CT, nc = min(a.CT, a.ncols - c0);
    const u64 e0 = (u64)epart * a.EP;
    const u32 ne = (u32)min((u64)a.EP, a.inner - e0);
    const u32 k0 = chunk * a.KC, kc = min(a.KC, a.U - k0);
    const u64 i0 = a.row0 + r0, j0 = a.col0 + c0;

    if (Staged) {
        stage(As, A, a.RT, nr, i0, a.inner, e0, 1ull, ne, a, a.ta, a.dTA, k0, kc);
        stage(Bs, B, a.CT, nc, j0, a.b_sk, e0, a.b_se, ne, a, a.tb, a.dTB, k0, kc);
        __syncthreads();
    }

    const u32 tt = a.ta * a.tb;
    const u32 len = a.RT * a.CT * a.EP * a.dTTKC.d;     // (row, column, e, a, b, unit), below 2^32 by the plan
    for (u32 l = threadIdx.x; l < len; l += 256u) {
        const u32 g = csgn_fastdiv(l, a.dTTKC), rem = l - g * a.dTTKC.d;
        const u32 ab = csgn_fastdiv(rem, a.dKC), kk = rem - ab * a.KC;
        const u32 ia = csgn_fastdiv(ab, a.dTB), ib = ab - ia * a.tb;
        const u32 rc = csgn_fastdiv(g, a.dEP), ee = g - rc * a.EP;
        const u32 rr = csgn_fastdiv(rc, a.dCT), cc = rc - rr * a.CT;
        if (rr >= nr || cc >= nc || ee >= ne || kk >= kc)
            continue;
        const u64 i = i0 + rr, j = j0 + cc, e = e0 + ee;
        Unit v;
        if (Staged)
            v = As[((rr * a.EP + ee) * a.ta + ia) * a.KC + kk] & Bs[((cc * a.EP + ee) * a.tb + ib) * a.KC + kk];
        else
            v = A[((i * a.inner + e) * a.ta + ia) * a.U + k0 + kk] &
                B[((e * a.b_se + j * a.b_sk) * a.tb + ib) * a.U + k0 + kk];
        unit_store<Unit, true>(C + (((i * a.cols + j) * a.inner + e) * tt + ab) * a.U + k0 + kk, v);
    }
}

// element p = (i * cols + k) * inner + e of the tiled operands: A's element i * inner + e, B's element e * b_se + k * b_sk
__global__ void __launch_bounds__(256) k_matmul_index(u64 p0, u64 np, u64 inner, u64 cols, u64 b_se, u64 b_sk,
                                                      u64 *__restrict__ ia, u64 *__restrict__ ib)
{
    for (u64 x = (u64)blockIdx.x * 256u + threadIdx.x; x < np; x += (u64)gridDim.x * 256u) {
        const u64 p = p0 + x, ik = p / inner, e = p - ik * inner, i = ik / cols, k = ik - i * cols;
        ia[x] = i * inner + e;
        ib[x] = e * b_se + k * b_sk;
    }
}

// ------------------------------------------------------------------------------ host side

bool matmul_shape_ok(u64 rows, u64 inner, u64 cols, u64 ta, u64 tb)
{
    return rows && cols && matmul_terms(inner, ta, tb) != 0;
}

// Per shape (measured): the fused kernel.  An operand of 2^32 elements or more is past what the gather
// launcher of the composed form takes: such a shape is fused whatever the knob says.
bool matmul_use_fused(u64 rows, u64 inner, u64 cols)
{
    unsigned long long na, nb;
    if (__builtin_mul_overflow((unsigned long long)rows, (unsigned long long)inner, &na) || na >= (1ull << 32) ||
        __builtin_mul_overflow((unsigned long long)inner, (unsigned long long)cols, &nb) || nb >= (1ull << 32))
        return true;
    return tune_choose(TUNE_MATMUL_FORM, true);
}

template <typename Unit>
hipError_t matmul_fused(u64 rows, u64 inner, u64 cols, const u64 *A, u64 ta, const u64 *B, u64 tb, bool transposed,
                        u64 *C, u32 U, hipStream_t st)
{
    const u64 ub = sizeof(Unit), tt = ta * tb;
    MatmulArgs a = {};
    a.A = A;
    a.B = B;
    a.C = C;
    a.inner = inner;
    a.cols = cols;
    a.b_se = transposed ? 1 : cols;
    a.b_sk = transposed ? inner : 1;
    a.ta = (u32)ta;
    a.tb = (u32)tb;
    a.U = U;
    // the slice of units: whole terms unless a 2 x 2 tile of them passes the budget
    u64 KC = U;
    if (2 * (ta + tb) * U * ub > kLdsBudget) {
        const u64 fit = kLdsBudget / (2 * (ta + tb) * ub);
        if (fit >= kMinChunk) {
            const u64 chunks = (U + fit - 1) / fit;
            KC = (U + chunks - 1) / chunks;
        }
    }
    a.KC = (u32)KC;
    a.chunks = (u32)((U + KC - 1) / KC);
    // the tile: rows and columns in turn while the staged terms of one e fit the budget and one output element's
    // stream of a workgroup stays below 2^32 units
    const u64 capR = std::min<u64>(rows, kMaxTile), capC = std::min<u64>(cols, kMaxTile);
    u64 RT = 1, CT = 1;
    for (;;) {
        const bool moreR = 2 * RT <= capR, moreC = 2 * CT <= capC;
        u64 nr = RT, nc = CT;
        if (moreR && (RT <= CT || !moreC))
            nr *= 2;
        else if (moreC)
            nc *= 2;
        else
            break;
        if ((nr * ta + nc * tb) * KC * ub > kLdsBudget || nr * nc * tt * KC > kMaxStream)
            break;
        RT = nr;
        CT = nc;
    }
    const bool staged = RT * CT > 1;
    if (!staged) {
        a.KC = U;
        a.chunks = 1;
        KC = U;
    }
    const u64 cell = RT * CT * tt * KC;                 // units of one e of a workgroup; tt * KC <= T * U < 2^31
    const u64 ctiles = (cols + CT - 1) / CT, rtiles = (rows + RT - 1) / RT;
    // the range of e: what the LDS holds, no more than kTargetUnits to write, parts enough to fill the chip, evened
    // out over the parts; or what knob matmul_epart says, which is how the tests choose the split
    const u64 capE = std::min<u64>({inner, kMaxStream / cell,
                                    staged ? kLdsBudget / ((RT * ta + CT * tb) * KC * ub) : inner});
    const u64 max_blocks = launch_blocks();
    const u64 minE = (inner * a.chunks + max_blocks - 1) / max_blocks;            // one tile's parts fit one launch
    u64 EP;
    const int forced = tune(TUNE_MATMUL_EPART);
    if (forced > 0) {
        EP = std::min<u64>((u64)forced, capE);
    } else {
        EP = std::min<u64>(capE, std::max<u64>(1, (kTargetUnits + cell - 1) / cell));
        while (EP > 1 && rtiles * ctiles * a.chunks * ((inner + EP - 1) / EP) < kFillBlocks &&
               ((EP + 1) / 2) * cell >= kMinUnits)
            EP = (EP + 1) / 2;
        const u64 parts = (inner + EP - 1) / EP;
        EP = (inner + parts - 1) / parts;
    }
    EP = std::max<u64>({EP, minE, 1});
    if (EP > capE)
        return hipErrorInvalidConfiguration;            // no shape within the C ABI's limits gets here
    a.RT = (u32)RT;
    a.CT = (u32)CT;
    a.EP = (u32)EP;
    a.eparts = (u32)((inner + EP - 1) / EP);
    a.dKC = csgn_fastdiv_make(a.KC);
    a.dTA = csgn_fastdiv_make(a.ta);
    a.dTB = csgn_fastdiv_make(a.tb);
    a.dTTKC = csgn_fastdiv_make((u32)(tt * KC));
    a.dEP = csgn_fastdiv_make(a.EP);
    a.dCT = csgn_fastdiv_make(a.CT);
    a.abase = (u32)((RT * EP * ta * KC * ub + 15u) & ~15ull);
    const u32 lds = staged ? a.abase + (u32)(CT * EP * tb * KC * ub) : 0u;
    a.xcd = stream_xcd(rows * cols * inner * tt * U);
    // columns of one launch: as many tiles as a launch's workgroups allow; rows by launch_groups
    const u64 per_tile = (u64)a.eparts * a.chunks;
    const u64 launch_ctiles = std::max<u64>(1, max_blocks / per_tile);
    for (u64 t0 = 0; t0 < ctiles; t0 += launch_ctiles) {
        const u64 nt = std::min(launch_ctiles, ctiles - t0);
        a.col0 = t0 * CT;
        a.ncols = (u32)std::min<u64>(cols - a.col0, nt * CT);
        a.ctiles = (u32)nt;
        const hipError_t err = launch_groups(max_blocks, rows, a.RT, nt * per_tile, [&](u64 r0, u64 nr, u32 nblocks) {
            a.row0 = r0;
            a.nrows = (u32)nr;
            a.nblocks = nblocks;
            if (staged)
                k_matmul<Unit, true><<<dim3(nblocks), 256, lds, st>>>(a);
            else
                k_matmul<Unit, false><<<dim3(nblocks), 256, 0, st>>>(a);
        });
        if (err != hipSuccess)
            return err;
    }
    return hipSuccess;
}

// The composed form through the tuned launchers: both operands tiled to rows * cols * inner elements by csgn_gather's
// launcher (element p = (i * cols + k) * inner + e: A's element i * inner + e, B's element e * cols + k), then ONE
// csgn_mul_uniform over those pairs straight into the output -- pair p's t_a * t_b terms, left term slow, are exactly
// terms [e * t_a * t_b, + t_a * t_b) of C[i,k].  The temporaries (the tiled operands and the two index lists) live in
// one block (scratch_take, csgn_kernels.h).  The gather takes fewer than 2^32 elements, so a larger product goes in
// slices of 2^31 pairs.
constexpr u64 kComposedSlice = 1ull << 31;

hipError_t matmul_composed(u64 n_bits, u64 rows, u64 inner, u64 cols, const u64 *A, u64 ta, const u64 *B, u64 tb,
                           bool transposed, u64 *C, hipStream_t st)
{
    const u64 dL = (n_bits + 63) / 64, pairs = rows * cols * inner, slice = std::min(pairs, kComposedSlice);
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *block = scratch_take(SCRATCH_MATMUL, slice * ((ta + tb) * dL + 2) * 8, st, owned, e);
    if (e != hipSuccess)
        return e;
    u64 *tiledA = block, *tiledB = block + slice * ta * dL, *ia = tiledB + slice * tb * dL, *ib = ia + slice;
    for (u64 p0 = 0; p0 < pairs && e == hipSuccess; p0 += slice) {
        const u64 np = std::min(slice, pairs - p0);
        const u32 blocks = (u32)std::min<u64>((np + 255) / 256, 8192);
        k_matmul_index<<<blocks, 256, 0, st>>>(p0, np, inner, cols, transposed ? 1 : cols, transposed ? inner : 1, ia, ib);
        e = hipGetLastError();
        if (e == hipSuccess)
            e = gather_planes(n_bits, 1, &A, &ta, rows * inner, np, ia, &tiledA, st);
        if (e == hipSuccess)
            e = gather_planes(n_bits, 1, &B, &tb, inner * cols, np, ib, &tiledB, st);
        if (e == hipSuccess)
            e = mul_uniform(n_bits, np, ta, tb, tiledA, tiledB, C + p0 * ta * tb * dL, 0, st);
    }
    return scratch_done(block, owned, e);
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 matmul_terms(u64 inner, u64 ta, u64 tb)
{
    u64 T = 0;
    if (inner == 0 || ta == 0 || tb == 0 || ta >= kTermLimit || tb >= kTermLimit || !term_mul(ta, tb, T) ||
        !term_mul(T, inner, T))
        return 0;
    return T;
}

const char *matmul_kernel_name(u64 n_bits, u64 rows, u64 inner, u64 cols, u64 ta, u64 tb, bool transposed)
{
    (void)transposed;
    if (n_bits == 0 || !matmul_shape_ok(rows, inner, cols, ta, tb))
        return "";
    return matmul_use_fused(rows, inner, cols) ? "k_matmul" : "composed";
}

hipError_t matmul(u64 n_bits, u64 rows, u64 inner, u64 cols, const u64 *A, u64 ta, const u64 *B, u64 tb,
                  bool transposed, u64 *C, hipStream_t stream)
{
    if (!matmul_use_fused(rows, inner, cols))
        return matmul_composed(n_bits, rows, inner, cols, A, ta, B, tb, transposed, C, stream);
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, A, B, C);
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? matmul_fused<unit16>(rows, inner, cols, A, ta, B, tb, transposed, C, U, stream)
                : matmul_fused<unit8>(rows, inner, cols, A, ta, B, tb, transposed, C, U, stream);
}

} // namespace csgn
