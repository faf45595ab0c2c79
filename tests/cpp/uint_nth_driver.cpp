// uint_nth_driver.cpp -- user-style C++ over nthWhere / takeWhere / nthIndex / nthSetIndex / atLeast / popcountAtLeast
// of include/certfhe/UInt.h: the k-th row whose encrypted mask bit is set (tests/test_uint_nth_cpp.py builds and runs
// it).
//   uint_nth_driver words   random masks with all-zero groups, every slot: decryptions == the (slot + 1)-th set row's
//                           value and index and "more than slot are set"; words == the definition composed from gather,
//                           operator* and operator+ (the "call" route against the explicit loop); takeWhere(k = g) gives
//                           the matching rows in order with valid bits 1...1 0...0; popcountAtLeast(a ^ b, k) against
//                           the plain Hamming distance
//   uint_nth_driver ragged  compacted (ragged) masks, values and integers, and integers whose planes differ in term
//                           count, take the "loop" route: words == the definition, elements the compaction left alone
//                           == the uniform operands' words; decryptions
//   uint_nth_driver errors  an output past 2^31 words per element throws before anything is allocated; bad groups,
//                           slots, k, planes, counts and contexts throw; empty batches give empty planes; atLeast at
//                           k = 0 and k > group; nthRoute
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "Gates.h"

#include <algorithm>
#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

struct Def {
    std::vector<CiphertextBatch> values, valid, labels;
    std::vector<bool> has;
};

// the definition of UInt.h, by hand from the batch operators: rows[r] = m_r, vrows[r][j] = plane j of value row r
Def definition(const std::vector<CiphertextBatch> &rows, const std::vector<std::vector<CiphertextBatch> > &vrows,
               const std::vector<uint64_t> &labels, unsigned planes, uint64_t slot)
{
    Def d;
    d.labels.assign(planes, rows[0]);
    d.has.assign(planes, false);
    for (uint64_t r = slot; r < rows.size(); ++r) {
        CiphertextBatch G = rows[r];
        bool first = true;
        for (uint64_t deg = slot; deg <= r; ++deg) {
            if (slot & ~deg)                                    // C(deg, slot) is even
                continue;
            // the deg-subsets of {0 .. r-1} in lexicographic order: the masks of r bits with deg set, bit i = row i,
            // ordered by their sorted member lists
            std::vector<std::vector<uint64_t> > subs;
            for (uint64_t m = 0; m < (1ull << r); ++m)
                if ((uint64_t)__builtin_popcountll(m) == deg) {
                    std::vector<uint64_t> s;
                    for (uint64_t i = 0; i < r; ++i)
                        if ((m >> i) & 1u)
                            s.push_back(i);
                    subs.push_back(s);
                }
            std::sort(subs.begin(), subs.end());
            for (const std::vector<uint64_t> &s : subs) {
                CiphertextBatch p = s.empty() ? rows[r] : rows[s[0]];
                for (size_t k = 1; k < s.size(); ++k)
                    p = p * rows[s[k]];
                if (!s.empty())
                    p = p * rows[r];
                G = first ? p : G + p;
                first = false;
            }
        }
        for (size_t j = 0; j < vrows[r].size(); ++j) {
            const CiphertextBatch p = G * vrows[r][j];
            if (r == slot)
                d.values.push_back(p);
            else
                d.values[j] = d.values[j] + p;
        }
        if (r == slot)
            d.valid.push_back(G);
        else
            d.valid[0] = d.valid[0] + G;
        for (unsigned i = 0; i < planes; ++i)
            if (!labels.empty() && ((labels[r] >> i) & 1u)) {
                d.labels[i] = d.has[i] ? d.labels[i] + G : G;
                d.has[i] = true;
            }
    }
    return d;
}

std::vector<uint64_t> rowIndex(uint64_t count, uint64_t g, uint64_t r)
{
    std::vector<uint64_t> idx(count);
    for (uint64_t q = 0; q < count; ++q)
        idx[q] = q * g + r;
    return idx;
}

// the rows of the grouped layout
Def grouped(const CiphertextBatch &mask, const UIntBatch *values, uint64_t g, const std::vector<uint64_t> &labels,
            unsigned planes, uint64_t slot)
{
    const uint64_t count = mask.size() / g;
    std::vector<CiphertextBatch> rows;
    std::vector<std::vector<CiphertextBatch> > vrows(g);
    for (uint64_t r = 0; r < g; ++r) {
        rows.push_back(mask.gather(rowIndex(count, g, r)));
        for (unsigned j = 0; values && j < values->width(); ++j)
            vrows[r].push_back(values->plane(j).gather(rowIndex(count, g, r)));
    }
    return definition(rows, vrows, labels, planes, slot);
}

// the planes of an integer as rows, bit 0 first
Def ofPlanes(const UIntBatch &a, const std::vector<uint64_t> &labels, unsigned planes, uint64_t slot)
{
    std::vector<CiphertextBatch> rows;
    for (unsigned r = 0; r < a.width(); ++r)
        rows.push_back(a.plane(r));
    return definition(rows, std::vector<std::vector<CiphertextBatch> >(a.width()), labels, planes, slot);
}

std::vector<uint64_t> indexLabels(unsigned g)
{
    std::vector<uint64_t> L(g);
    for (unsigned r = 0; r < g; ++r)
        L[r] = r;
    return L;
}

// plane i of `got` against the definition's: its words where some label reaches the plane, else one ZERO term
void checkLabels(const UIntBatch &got, const Def &d, const SecretKey &key, const std::string &tag, uint64_t from = 0)
{
    expect(got.width() == d.labels.size(), "label planes" + tag);
    for (unsigned i = 0; i < got.width() && i < d.labels.size(); ++i) {
        if (d.has[i]) {
            bool same = got.plane(i).size() == d.labels[i].size();
            for (uint64_t q = from; q < got.size() && same; ++q)
                same = sameWords(got.plane(i).at(q), d.labels[i].at(q));
            expect(same, "label plane " + std::to_string(i) + " words == definition" + tag);
        } else {
            const std::vector<unsigned char> bits = got.plane(i).decrypt(key);
            expect(got.plane(i).uniform() && got.plane(i).terms() == 1 &&
                       std::count(bits.begin(), bits.end(), 0) == (long)bits.size(),
                   "label plane " + std::to_string(i) + " is the one-term ZERO" + tag);
        }
    }
}

bool sameFrom(const CiphertextBatch &x, const CiphertextBatch &y, uint64_t from)
{
    bool same = x.size() == y.size();
    for (uint64_t q = from; q < x.size() && same; ++q)
        same = sameWords(x.at(q), y.at(q));
    return same;
}

struct Case {
    unsigned g, w;
    size_t count;
};
const Case kCases[] = {{1, 3, 7}, {3, 4, 50}, {4, 8, 60}, {6, 2, 20}};

// masks with all-zero groups and the clear results of one slot
struct Clear {
    std::vector<unsigned char> bits;
    std::vector<uint64_t> vals;
};
Clear clearCase(const Case &c)
{
    Clear x;
    x.bits.resize(c.count * c.g);
    x.vals.resize(c.count * c.g);
    for (size_t q = 0; q < c.count; ++q)
        for (unsigned r = 0; r < c.g; ++r) {
            x.bits[q * c.g + r] = q % 3 == 0 ? 0 : (unsigned char)rnd(1);
            x.vals[q * c.g + r] = rnd(c.w);
        }
    return x;
}
struct Slot {
    std::vector<uint64_t> want, index, valid;
};
Slot clearSlot(const Case &c, const Clear &x, uint64_t slot)
{
    Slot s;
    s.want.assign(c.count, 0);
    s.index.assign(c.count, 0);
    s.valid.assign(c.count, 0);
    for (size_t q = 0; q < c.count; ++q) {
        uint64_t seen = 0;
        for (unsigned r = 0; r < c.g; ++r)
            if (x.bits[q * c.g + r] && seen++ == slot) {
                s.want[q] = x.vals[q * c.g + r];
                s.index[q] = r;
                s.valid[q] = 1;
            }
    }
    return s;
}

void checkBits(const CiphertextBatch &got, const std::vector<uint64_t> &want, const SecretKey &key, const std::string &tag)
{
    const std::vector<unsigned char> bits = got.decrypt(key);
    bool same = bits.size() == want.size();
    for (size_t i = 0; i < bits.size() && same; ++i)
        same = bits[i] == want[i];
    expect(same, tag);
}

// the position of the (slot + 1)-th set bit of x, 0 and not valid where there is none
uint64_t nthBit(uint64_t x, uint64_t slot, uint64_t *valid)
{
    for (unsigned r = 0; r < 64; ++r)
        if ((x >> r) & 1u) {
            if (slot == 0) {
                *valid = 1;
                return r;
            }
            --slot;
        }
    *valid = 0;
    return 0;
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    for (const Case &c : kCases) {
        const Clear x = clearCase(c);
        const CiphertextBatch mask = CiphertextBatch::encrypt(key, x.bits, 20 + c.g);
        const UIntBatch vals = UIntBatch::encrypt(key, x.vals, c.w, 21 + c.g);
        const unsigned planes = 4;
        std::vector<CiphertextBatch> all_valid;
        const std::vector<UIntBatch> taken = takeWhere(mask, vals, c.g, c.g, &all_valid);
        expect(taken.size() == c.g && all_valid.size() == c.g, "takeWhere(k = g) gives g slots");
        expect(takeWhere(mask, vals, c.g, 1).size() == 1, "takeWhere(k = 1) without valid");
        for (uint64_t slot = 0; slot < c.g; ++slot) {
            const std::string tag = " g=" + std::to_string(c.g) + " w=" + std::to_string(c.w) + " slot=" + std::to_string(slot);
            expect(std::string(nthRoute(c.g, mask.uniform())) == "call", "uniform operands take the call" + tag);
            const Slot s = clearSlot(c, x, slot);
            const Def d = grouped(mask, &vals, c.g, indexLabels(c.g), planes, slot);
            CiphertextBatch valid = mask;
            const UIntBatch r = nthWhere(mask, vals, c.g, slot, &valid);
            checkValues(r.decrypt(key), s.want, "nthWhere" + tag);
            checkBits(valid, s.valid, key, "valid" + tag);
            expect(sameWords(r, UIntBatch::fromPlanes(d.values)), "nthWhere words == definition" + tag);
            expect(sameBatchWords(valid, d.valid[0]), "valid words == definition" + tag);
            expect(sameWords(nthWhere(mask, vals, c.g, slot), r), "nthWhere without valid" + tag);
            CiphertextBatch valid2 = mask;
            expect(sameBatchWords(nthWhere(mask, vals.plane(c.w - 1), c.g, slot, &valid2), d.values[c.w - 1]) &&
                       sameBatchWords(valid2, d.valid[0]),
                   "the batch overload, with valid" + tag);
            expect(sameBatchWords(nthWhere(mask, vals.plane(0), c.g, slot), d.values[0]), "the batch overload" + tag);
            expect(sameBatchWords(atLeast(mask, c.g, slot + 1), d.valid[0]), "atLeast words == definition" + tag);
            CiphertextBatch valid3 = mask;
            const UIntBatch ni = nthIndex(mask, c.g, slot, planes, &valid3);
            checkValues(ni.decrypt(key), s.index, "nthIndex" + tag);
            checkLabels(ni, d, key, " nthIndex" + tag);
            expect(sameBatchWords(valid3, d.valid[0]), "nthIndex valid" + tag);
            checkLabels(nthIndex(mask, c.g, slot, planes), d, key, " nthIndex without valid" + tag);
            // takeWhere: the matching rows in order, the valid bits 1...1 0...0
            if (slot < taken.size()) {
                expect(sameWords(taken[slot], r), "takeWhere slot words == nthWhere" + tag);
                expect(sameBatchWords(all_valid[slot], valid), "takeWhere valid words == nthWhere" + tag);
                checkValues(taken[slot].decrypt(key), s.want, "takeWhere" + tag);
                checkBits(all_valid[slot], s.valid, key, "takeWhere valid" + tag);
            }
        }
        // a public answer costs no terms
        const CiphertextBatch all = atLeast(mask, c.g, 0), none = atLeast(mask, c.g, c.g + 1);
        expect(all.size() == c.count && all.uniform() && all.terms() == 1 && none.size() == c.count && none.uniform() &&
                   none.terms() == 1,
               "atLeast at k = 0 and k > group: one term");
        checkBits(all, std::vector<uint64_t>(c.count, 1), key, "atLeast(k = 0) is ONE");
        checkBits(none, std::vector<uint64_t>(c.count, 0), key, "atLeast(k > group) is ZERO");
    }
    // an integer's own planes: widths 1 (one grouped batch of groups of 1), 5 and 8
    for (unsigned w : {1u, 5u, 8u}) {
        const size_t count = 40;
        std::vector<uint64_t> a(count), b(count);
        for (size_t i = 0; i < count; ++i) {
            a[i] = i % 4 == 0 ? 0 : rnd(w) >> (i % w);
            b[i] = rnd(w);
        }
        const UIntBatch x = UIntBatch::encrypt(key, a, w, 40 + w), y = UIntBatch::encrypt(key, b, w, 50 + w);
        const unsigned planes = 4;
        for (uint64_t slot = 0; slot < w; ++slot) {
            const std::string tag = " width=" + std::to_string(w) + " slot=" + std::to_string(slot);
            std::vector<uint64_t> pos(count), ok(count), ge(count);
            for (size_t i = 0; i < count; ++i) {
                pos[i] = nthBit(a[i], slot, &ok[i]);
                ge[i] = (uint64_t)__builtin_popcountll(a[i]) >= slot + 1;
            }
            CiphertextBatch valid = x.plane(0);
            const UIntBatch si = nthSetIndex(x, slot, planes, &valid);
            const Def d = ofPlanes(x, indexLabels(w), planes, slot);
            checkValues(si.decrypt(key), pos, "nthSetIndex" + tag);
            checkBits(valid, ok, key, "nthSetIndex valid" + tag);
            checkLabels(si, d, key, " nthSetIndex" + tag);
            expect(sameBatchWords(valid, d.valid[0]), "nthSetIndex valid words == definition" + tag);
            checkLabels(nthSetIndex(x, slot, planes), d, key, " nthSetIndex without valid" + tag);
            const CiphertextBatch pa = popcountAtLeast(x, slot + 1);
            expect(sameBatchWords(pa, d.valid[0]), "popcountAtLeast words == definition" + tag);
            checkBits(pa, ge, key, "popcountAtLeast" + tag);
        }
        // the Hamming-distance threshold, through a ^ b (planes of 2 terms: one term count, the call)
        for (uint64_t k = 0; k <= w + 1; k += (w > 5 ? 3 : 1)) {
            std::vector<uint64_t> far(count);
            for (size_t i = 0; i < count; ++i)
                far[i] = (uint64_t)__builtin_popcountll(a[i] ^ b[i]) >= k;
            checkBits(popcountAtLeast(x ^ y, k), far, key,
                      "popcountAtLeast(a ^ b, " + std::to_string(k) + ") width=" + std::to_string(w));
        }
    }
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    // batch + p + q, compacted: element 0 keeps [a, ONE, ZERO] (its bit flips), every other element adds ZERO twice,
    // which cancels: it holds exactly the uniform batch's term.  The batch is ragged.
    auto raggedOf = [&](const CiphertextBatch &a) {
        std::vector<unsigned char> p(a.size(), 0), q(a.size(), 0);
        p[0] = 1;
        return addPlain(addPlain(a, p), q).compact();
    };
    auto raggedInt = [&](const UIntBatch &a) {
        std::vector<CiphertextBatch> pr;
        for (unsigned j = 0; j < a.width(); ++j)
            pr.push_back(raggedOf(a.plane(j)));
        return UIntBatch::fromPlanes(pr);
    };
    for (const Case &c : {Case{2, 3, 30}, Case{4, 2, 25}, Case{5, 3, 12}}) {
        Clear x = clearCase(c);
        x.bits[0] = 0;                                               // flipped to 1 by the compaction
        const CiphertextBatch mask = CiphertextBatch::encrypt(key, x.bits, 60 + c.g);
        const UIntBatch vals = UIntBatch::encrypt(key, x.vals, c.w, 61 + c.g);
        const CiphertextBatch mr = raggedOf(mask);
        const UIntBatch vr = raggedInt(vals);
        Clear xm = x;
        xm.bits[0] = 1;
        Clear xv = x;
        for (unsigned r = 0; r < c.g; ++r)                           // element 0 of every value plane flips: rows 0..g-1
            xv.vals[r] ^= r == 0 ? (1ull << c.w) - 1 : 0;
        const unsigned planes = 3;
        for (uint64_t slot = 0; slot < c.g; ++slot) {
            const std::string tag = " g=" + std::to_string(c.g) + " slot=" + std::to_string(slot);
            expect(!mr.uniform() && !vr.plane(0).uniform(), "compact() gave ragged operands" + tag);
            expect(std::string(nthRoute(c.g, mr.uniform())) == "loop", "ragged operands take the loop" + tag);
            CiphertextBatch valid = mask, validu = mask;
            const UIntBatch uni = nthWhere(mask, vals, c.g, slot, &validu), uidx = nthIndex(mask, c.g, slot, planes);
            // a ragged mask
            const Slot sm = clearSlot(c, xm, slot);
            const Def dm = grouped(mr, &vals, c.g, indexLabels(c.g), planes, slot);
            const UIntBatch rm = nthWhere(mr, vals, c.g, slot, &valid);
            expect(sameWords(rm, UIntBatch::fromPlanes(dm.values)), "ragged mask: words == definition" + tag);
            expect(sameBatchWords(valid, dm.valid[0]), "ragged mask: valid == definition" + tag);
            expect(sameBatchWords(atLeast(mr, c.g, slot + 1), dm.valid[0]), "ragged mask: atLeast == definition" + tag);
            checkValues(rm.decrypt(key), sm.want, "ragged mask" + tag);
            checkBits(valid, sm.valid, key, "ragged mask: valid" + tag);
            const UIntBatch ri = nthIndex(mr, c.g, slot, planes);
            checkLabels(ri, dm, key, " ragged mask: nthIndex" + tag);
            checkValues(ri.decrypt(key), sm.index, "ragged mask: nthIndex" + tag);
            // output elements 1.. hold the uniform operands' terms, so the same words as the call's
            for (unsigned j = 0; j < c.w; ++j)
                expect(sameFrom(rm.plane(j), uni.plane(j), 1), "loop words == call words" + tag);
            expect(sameFrom(valid, validu, 1), "loop valid == call valid" + tag);
            for (unsigned i = 0; i < planes; ++i)
                if (dm.has[i])
                    expect(sameFrom(ri.plane(i), uidx.plane(i), 1), "loop index == call index" + tag);
            // ragged values
            const Slot sv = clearSlot(c, xv, slot);
            const Def dv = grouped(mask, &vr, c.g, std::vector<uint64_t>(), 0, slot);
            const UIntBatch rv = nthWhere(mask, vr, c.g, slot);
            expect(sameWords(rv, UIntBatch::fromPlanes(dv.values)), "ragged values: words == definition" + tag);
            checkValues(rv.decrypt(key), sv.want, "ragged values" + tag);
            expect(sameBatchWords(nthWhere(mask, vr.plane(0), c.g, slot), dv.values[0]),
                   "ragged values: the batch overload" + tag);
            for (unsigned j = 0; j < c.w; ++j)
                expect(sameFrom(rv.plane(j), uni.plane(j), 1), "ragged values: loop words == call words" + tag);
        }
        std::vector<CiphertextBatch> tv;
        const std::vector<UIntBatch> taken = takeWhere(mr, vals, c.g, c.g, &tv);
        for (uint64_t slot = 0; slot < c.g; ++slot) {
            const Slot sm = clearSlot(c, xm, slot);
            checkValues(taken[slot].decrypt(key), sm.want, "ragged takeWhere slot " + std::to_string(slot));
            checkBits(tv[slot], sm.valid, key, "ragged takeWhere valid slot " + std::to_string(slot));
        }
    }
    // an integer of ragged planes (element 0 is the complement), and one of UNIFORM planes of different term counts: a
    // sum's plane j has more terms than plane j - 1.  Both take the loop.
    for (unsigned w : {3u, 5u}) {
        const size_t count = 20;
        std::vector<uint64_t> a(count), b(count), sum(count);
        for (size_t i = 0; i < count; ++i) {
            a[i] = i % 4 == 0 ? 0 : rnd(w) >> (i % w);
            b[i] = rnd(w);
            sum[i] = (a[i] + b[i]) & ((1ull << w) - 1);
        }
        const UIntBatch x0 = UIntBatch::encrypt(key, a, w, 80 + w), xr = raggedInt(x0);
        const UIntBatch xs = x0 + UIntBatch::encrypt(key, b, w, 90 + w);
        expect(xs.plane(0).uniform() && xs.plane(w - 1).uniform() && xs.plane(w - 1).terms() != xs.plane(0).terms(),
               "a sum's planes are uniform with different term counts");
        a[0] ^= (1ull << w) - 1;
        const unsigned planes = 3;
        for (uint64_t slot = 0; slot < w; ++slot) {
            const std::string tag = " ragged width=" + std::to_string(w) + " slot=" + std::to_string(slot);
            std::vector<uint64_t> pos(count), ok(count), spos(count), sok(count);
            for (size_t i = 0; i < count; ++i) {
                pos[i] = nthBit(a[i], slot, &ok[i]) & ((1u << planes) - 1);
                spos[i] = nthBit(sum[i], slot, &sok[i]) & ((1u << planes) - 1);
            }
            CiphertextBatch valid = xr.plane(0);
            const UIntBatch si = nthSetIndex(xr, slot, planes, &valid);
            const Def d = ofPlanes(xr, indexLabels(w), planes, slot);
            checkValues(si.decrypt(key), pos, "nthSetIndex" + tag);
            checkBits(valid, ok, key, "nthSetIndex valid" + tag);
            checkLabels(si, d, key, " nthSetIndex" + tag);
            expect(sameBatchWords(valid, d.valid[0]), "nthSetIndex valid == definition" + tag);
            expect(sameBatchWords(popcountAtLeast(xr, slot + 1), d.valid[0]), "popcountAtLeast == definition" + tag);
            // elements 1.. against the call on the uniform integer
            checkLabels(si, ofPlanes(x0, indexLabels(w), planes, slot), key, " loop == call: nthSetIndex" + tag, 1);
            expect(sameFrom(valid, popcountAtLeast(x0, slot + 1), 1), "loop == call: popcountAtLeast" + tag);
            // planes of different term counts (the narrow sum only: the size check takes the largest count for every
            // row, and the wider sum's top plane to the fifth power is past the limit)
            if (w == 3) {
                CiphertextBatch svalid = xs.plane(0);
                const UIntBatch ss = nthSetIndex(xs, slot, planes, &svalid);
                const Def ds = ofPlanes(xs, indexLabels(w), planes, slot);
                checkValues(ss.decrypt(key), spos, "mixed term counts: nthSetIndex" + tag);
                checkBits(svalid, sok, key, "mixed term counts: valid" + tag);
                checkLabels(ss, ds, key, " mixed term counts: nthSetIndex" + tag);
                expect(sameBatchWords(svalid, ds.valid[0]), "mixed term counts: valid == definition" + tag);
            }
        }
    }
    return 0;
}

// Groups of 32 fresh rows at N=1247: slot 0 has 2^32 - 1 entries.  The size check comes first, so the call throws
// std::invalid_argument at once, before any allocation or launch.
int errors()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const size_t count = 320;
    const CiphertextBatch mask = CiphertextBatch::encrypt(key, randomBits(count), 1);
    const UIntBatch vals = UIntBatch::encrypt(key, std::vector<uint64_t>(count, 3), 2, 2);
    const UIntBatch wide = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 5), 32, 3);
    const auto t0 = std::chrono::steady_clock::now();
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { nthWhere(mask, vals, 32, 0); });
    thrown += throws<std::invalid_argument>([&] { nthWhere(mask, vals.plane(0), 32, 1); });
    thrown += throws<std::invalid_argument>([&] { atLeast(mask, 32, 2); });
    thrown += throws<std::invalid_argument>([&] { nthIndex(mask, 32, 3, 5); });
    thrown += throws<std::invalid_argument>([&] { nthWhere(mask, vals, 64, 0); });      // 2^64 - 1 entries
    thrown += throws<std::invalid_argument>([&] { takeWhere(mask, vals, 32, 32); });    // slot 31 alone would fit
    thrown += throws<std::invalid_argument>([&] { nthSetIndex(wide, 0, 5); });
    thrown += throws<std::invalid_argument>([&] { popcountAtLeast(wide, 16); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 8, "oversize throws (" + std::to_string(thrown) + " of 8)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    // the high slots of wide groups are small: 32 rows at slot 30 have C(32, 31) + C(32, 32) = 33 entries
    checkBits(atLeast(mask, 32, 32), std::vector<uint64_t>(count / 32, 0), key, "atLeast(32 of 32) of random bits");
    expect(atLeast(mask, 32, 31).terms() == 33 && popcountAtLeast(wide, 32).terms() == 1, "the high slots stay small");
    // groups, slots, k, planes, counts, contexts
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { nthWhere(mask, vals, 0, 0); });                       // groups
    thrown += throws<std::invalid_argument>([&] { nthWhere(mask, vals, 65, 0); });
    thrown += throws<std::invalid_argument>([&] { nthWhere(mask, vals, 3, 0); });                       // 320 % 3
    thrown += throws<std::invalid_argument>([&] { atLeast(mask, 0, 1); });
    thrown += throws<std::invalid_argument>([&] { atLeast(mask, 7, 1); });
    thrown += throws<std::invalid_argument>([&] { atLeast(mask, 7, 0); });                              // also at a public k
    thrown += throws<std::invalid_argument>([&] { atLeast(mask, 65, 66); });
    thrown += throws<std::invalid_argument>([&] { nthIndex(mask, 65, 0, 3); });
    thrown += throws<std::invalid_argument>([&] { nthWhere(mask, vals, 4, 4); });                       // slots
    thrown += throws<std::invalid_argument>([&] { nthWhere(mask, vals.plane(0), 4, 9); });
    thrown += throws<std::invalid_argument>([&] { nthIndex(mask, 4, 4, 3); });
    thrown += throws<std::invalid_argument>([&] { nthSetIndex(vals, 2, 3); });
    thrown += throws<std::invalid_argument>([&] { takeWhere(mask, vals, 4, 0); });                      // k
    thrown += throws<std::invalid_argument>([&] { takeWhere(mask, vals, 4, 5); });
    thrown += throws<std::invalid_argument>([&] { nthIndex(mask, 4, 1, 0); });                          // planes
    thrown += throws<std::invalid_argument>([&] { nthIndex(mask, 4, 1, 65); });
    thrown += throws<std::invalid_argument>([&] { nthSetIndex(vals, 0, 0); });
    thrown += throws<std::invalid_argument>([&] { nthSetIndex(vals, 0, 65); });
    thrown += throws<std::invalid_argument>([&] { nthWhere(mask, vals.slice(0, 316), 4, 1); });         // counts
    thrown += throws<std::invalid_argument>([&] { nthWhere(mask.slice(0, 316), vals.plane(0), 4, 1); });
    Context other(127, 8);
    SecretKey okey(other);
    thrown += throws<std::invalid_argument>([&] { nthWhere(mask, UIntBatch::encrypt(okey, std::vector<uint64_t>(count, 1), 2, 9), 4, 1); });
    thrown += throws<std::invalid_argument>([&] { nthWhere(CiphertextBatch::encrypt(okey, randomBits(count), 9), vals.plane(1), 4, 1); });
    expect(thrown == 22, "bad groups, slots, k, planes, counts and contexts throw (" + std::to_string(thrown) + " of 22)");
    // empty batches: empty planes
    CiphertextBatch valid = mask;
    const UIntBatch none = nthWhere(mask.slice(0, 0), vals.slice(0, 0), 4, 2, &valid);
    expect(none.width() == 2 && none.size() == 0 && valid.size() == 0, "an empty batch gives empty planes");
    expect(atLeast(mask.slice(0, 0), 8, 3).size() == 0 && atLeast(mask.slice(0, 0), 8, 0).size() == 0 &&
               atLeast(mask.slice(0, 0), 8, 9).size() == 0,
           "atLeast of an empty batch");
    const UIntBatch ni = nthIndex(mask.slice(0, 0), 8, 7, 5, &valid);
    expect(ni.width() == 5 && ni.size() == 0 && valid.size() == 0, "nthIndex of an empty batch");
    std::vector<CiphertextBatch> tv;
    const std::vector<UIntBatch> te = takeWhere(mask.slice(0, 0), vals.slice(0, 0), 4, 3, &tv);
    expect(te.size() == 3 && tv.size() == 3 && te[2].width() == 2 && te[2].size() == 0 && tv[2].size() == 0,
           "takeWhere of an empty batch");
    const UIntBatch e = vals.slice(0, 0);
    expect(nthSetIndex(e, 1, 3).width() == 3 && nthSetIndex(e, 1, 3).size() == 0 && popcountAtLeast(e, 1).size() == 0 &&
               popcountAtLeast(e, 0).size() == 0,
           "an empty integer gives empty planes");
    // the routes
    expect(std::string(nthRoute(8, true)) == "call" && std::string(nthRoute(1, true)) == "call" &&
               std::string(nthRoute(64, true)) == "call",
           "uniform operands: the call");
    expect(std::string(nthRoute(8, false)) == "loop" && std::string(nthRoute(0, true)) == "loop" &&
               std::string(nthRoute(65, true)) == "loop",
           "ragged operands or a group the call refuses: the loop");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 5233, "uint_nth_driver", {{"words", words}, {"ragged", ragged}, {"errors", errors}});
}
