// uint_first_driver.cpp -- user-style C++ over firstWhere / anyOf / firstIndex / lowestSetIndex / lowestSetBit /
// bitLength of include/certfhe/UInt.h: the first row whose encrypted mask bit is set (tests/test_uint_first_cpp.py builds
// and runs it).
//   uint_first_driver words   random masks with all-zero groups: decryptions == the first set row's value, the OR, the
//                             index, the lowest set bit and the bit length; words == the definition composed from
//                             gather, logicNot, operator* and operator+ (the "call" route against the explicit loop)
//   uint_first_driver ragged  compacted (ragged) masks, values and integers take the "loop" route: words == the
//                             definition, elements the compaction left alone == the uniform operands' words; decryptions
//   uint_first_driver errors  an output past 2^31 words per element throws before anything is allocated; bad groups,
//                             planes, counts and contexts throw; empty batches give empty planes; firstRoute
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "Gates.h"

#include <algorithm>
#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

struct Def {
    std::vector<CiphertextBatch> values, any, labels;
    std::vector<bool> has;
};

// the definition of UInt.h, by hand from the batch operators: rows[r] = m_r, vrows[r][j] = plane j of value row r
Def definition(const std::vector<CiphertextBatch> &rows, const std::vector<std::vector<CiphertextBatch> > &vrows,
               const std::vector<uint64_t> &labels, unsigned planes)
{
    Def d;
    d.labels.assign(planes, rows[0]);
    d.has.assign(planes, false);
    CiphertextBatch run = rows[0];
    for (size_t r = 0; r < rows.size(); ++r) {
        const CiphertextBatch F = r == 0 ? rows[0] : run * rows[r];
        if (r + 1 < rows.size())
            run = r == 0 ? logicNot(rows[0]) : run * logicNot(rows[r]);
        for (size_t j = 0; j < vrows[r].size(); ++j) {
            const CiphertextBatch p = F * vrows[r][j];
            if (r == 0)
                d.values.push_back(p);
            else
                d.values[j] = d.values[j] + p;
        }
        if (r == 0)
            d.any.push_back(F);
        else
            d.any[0] = d.any[0] + F;
        for (unsigned i = 0; i < planes; ++i)
            if (!labels.empty() && ((labels[r] >> i) & 1u)) {
                d.labels[i] = d.has[i] ? d.labels[i] + F : F;
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
            unsigned planes)
{
    const uint64_t count = mask.size() / g;
    std::vector<CiphertextBatch> rows;
    std::vector<std::vector<CiphertextBatch> > vrows(g);
    for (uint64_t r = 0; r < g; ++r) {
        rows.push_back(mask.gather(rowIndex(count, g, r)));
        for (unsigned j = 0; values && j < values->width(); ++j)
            vrows[r].push_back(values->plane(j).gather(rowIndex(count, g, r)));
    }
    return definition(rows, vrows, labels, planes);
}

// the planes of an integer as rows, bit 0 first or from the top
Def ofPlanes(const UIntBatch &a, bool from_top, const std::vector<uint64_t> &labels, unsigned planes)
{
    std::vector<CiphertextBatch> rows;
    for (unsigned r = 0; r < a.width(); ++r)
        rows.push_back(a.plane(from_top ? a.width() - 1 - r : r));
    return definition(rows, std::vector<std::vector<CiphertextBatch> >(a.width()), labels, planes);
}

std::vector<uint64_t> labelsOf(unsigned g, int kind)      // 0: r, 1: 1 << r, 2: g - r
{
    std::vector<uint64_t> L(g);
    for (unsigned r = 0; r < g; ++r)
        L[r] = kind == 0 ? r : kind == 1 ? 1ull << r : g - r;
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

unsigned lowest(uint64_t x) { return x ? (unsigned)__builtin_ctzll(x) : 0; }
unsigned length(uint64_t x) { return x ? 64 - (unsigned)__builtin_clzll(x) : 0; }

struct Case {
    unsigned g, w;
    size_t count;
};
const Case kCases[] = {{1, 3, 7}, {3, 4, 50}, {4, 8, 100}, {8, 5, 20}, {6, 2, 33}};

// masks with all-zero groups and the clear results
struct Clear {
    std::vector<unsigned char> bits;
    std::vector<uint64_t> vals, want, index, any;
};
Clear clearCase(const Case &c)
{
    Clear x;
    x.bits.resize(c.count * c.g);
    x.vals.resize(c.count * c.g);
    x.want.assign(c.count, 0);
    x.index.assign(c.count, 0);
    x.any.assign(c.count, 0);
    for (size_t q = 0; q < c.count; ++q)
        for (unsigned r = 0; r < c.g; ++r) {
            x.bits[q * c.g + r] = q % 3 == 0 ? 0 : (unsigned char)rnd(1);
            x.vals[q * c.g + r] = rnd(c.w);
            if (x.bits[q * c.g + r] && !x.any[q]) {
                x.any[q] = 1;
                x.index[q] = r;
                x.want[q] = x.vals[q * c.g + r];
            }
        }
    return x;
}

void checkBits(const CiphertextBatch &got, const std::vector<uint64_t> &want, const SecretKey &key, const std::string &tag)
{
    const std::vector<unsigned char> bits = got.decrypt(key);
    bool same = bits.size() == want.size();
    for (size_t i = 0; i < bits.size() && same; ++i)
        same = bits[i] == want[i];
    expect(same, tag);
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    for (const Case &c : kCases) {
        const Clear x = clearCase(c);
        const CiphertextBatch mask = CiphertextBatch::encrypt(key, x.bits, 20 + c.g);
        const UIntBatch vals = UIntBatch::encrypt(key, x.vals, c.w, 21 + c.g);
        const std::string tag = " g=" + std::to_string(c.g) + " w=" + std::to_string(c.w);
        expect(std::string(firstRoute(c.g, mask.uniform())) == "call", "uniform operands take the call" + tag);
        const unsigned planes = 4;
        const Def d = grouped(mask, &vals, c.g, labelsOf(c.g, 0), planes);
        CiphertextBatch any = mask;
        const UIntBatch r = firstWhere(mask, vals, c.g, &any);
        checkValues(r.decrypt(key), x.want, "firstWhere" + tag);
        checkBits(any, x.any, key, "any" + tag);
        expect(sameWords(r, UIntBatch::fromPlanes(d.values)), "firstWhere words == definition" + tag);
        expect(sameBatchWords(any, d.any[0]), "any words == definition" + tag);
        expect(sameWords(firstWhere(mask, vals, c.g), r), "firstWhere without any" + tag);
        CiphertextBatch any2 = mask;
        expect(sameBatchWords(firstWhere(mask, vals.plane(c.w - 1), c.g, &any2), d.values[c.w - 1]) &&
                   sameBatchWords(any2, d.any[0]),
               "the batch overload, with any" + tag);
        expect(sameBatchWords(firstWhere(mask, vals.plane(0), c.g), d.values[0]), "the batch overload" + tag);
        expect(sameBatchWords(anyOf(mask, c.g), d.any[0]), "anyOf words == definition" + tag);
        CiphertextBatch any3 = mask;
        const UIntBatch fi = firstIndex(mask, c.g, planes, &any3);
        checkValues(fi.decrypt(key), x.index, "firstIndex" + tag);
        checkLabels(fi, d, key, " firstIndex" + tag);
        expect(sameBatchWords(any3, d.any[0]), "firstIndex any" + tag);
        checkLabels(firstIndex(mask, c.g, planes), d, key, " firstIndex without any" + tag);
    }
    // an integer's own planes: widths 1 (one grouped batch of groups of 1), 5, 8 and 16
    for (unsigned w : {1u, 5u, 8u, 16u}) {
        const size_t count = w == 16 ? 3 : 40;
        std::vector<uint64_t> a(count), lo(count), bit(count), len(count), nz(count);
        for (size_t i = 0; i < count; ++i) {
            a[i] = i % 4 == 0 ? 0 : rnd(w) >> (i % w);
            lo[i] = lowest(a[i]);
            bit[i] = a[i] & (~a[i] + 1);
            len[i] = length(a[i]);
            nz[i] = a[i] != 0;
        }
        const UIntBatch x = UIntBatch::encrypt(key, a, w, 40 + w);
        const std::string tag = " width=" + std::to_string(w);
        const unsigned planes = 5;
        CiphertextBatch nonzero = x.plane(0);
        const UIntBatch li = lowestSetIndex(x, planes, &nonzero);
        const Def di = ofPlanes(x, false, labelsOf(w, 0), planes);
        checkValues(li.decrypt(key), lo, "lowestSetIndex" + tag);
        checkBits(nonzero, nz, key, "nonzero" + tag);
        checkLabels(li, di, key, " lowestSetIndex" + tag);
        expect(sameBatchWords(nonzero, di.any[0]), "nonzero words == definition" + tag);
        checkLabels(lowestSetIndex(x, planes), di, key, " lowestSetIndex without nonzero" + tag);
        const UIntBatch lb = lowestSetBit(x);
        checkValues(lb.decrypt(key), bit, "lowestSetBit" + tag);
        checkLabels(lb, ofPlanes(x, false, labelsOf(w, 1), w), key, " lowestSetBit" + tag);
        const UIntBatch bl = bitLength(x, planes);
        checkValues(bl.decrypt(key), len, "bitLength" + tag);
        checkLabels(bl, ofPlanes(x, true, labelsOf(w, 2), planes), key, " bitLength" + tag);
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
    for (const Case &c : {Case{2, 3, 30}, Case{4, 2, 25}, Case{5, 4, 12}}) {
        Clear x = clearCase(c);
        x.bits[0] = 0;                                               // flipped to 1 by the compaction: row 0 is the first
        const CiphertextBatch mask = CiphertextBatch::encrypt(key, x.bits, 60 + c.g);
        const UIntBatch vals = UIntBatch::encrypt(key, x.vals, c.w, 61 + c.g);
        const CiphertextBatch mr = raggedOf(mask);
        const UIntBatch vr = raggedInt(vals);
        const std::string tag = " g=" + std::to_string(c.g);
        expect(!mr.uniform() && !vr.plane(0).uniform(), "compact() gave ragged operands" + tag);
        expect(std::string(firstRoute(c.g, mr.uniform())) == "loop", "ragged operands take the loop" + tag);
        const unsigned planes = 3;
        CiphertextBatch any = mask, anyu = mask;
        const UIntBatch uni = firstWhere(mask, vals, c.g, &anyu), uidx = firstIndex(mask, c.g, planes);
        // a ragged mask
        std::vector<uint64_t> want = x.want, index = x.index, anyw = x.any;
        want[0] = x.vals[0];
        index[0] = 0;
        anyw[0] = 1;
        const Def dm = grouped(mr, &vals, c.g, labelsOf(c.g, 0), planes);
        const UIntBatch rm = firstWhere(mr, vals, c.g, &any);
        expect(sameWords(rm, UIntBatch::fromPlanes(dm.values)), "ragged mask: words == definition" + tag);
        expect(sameBatchWords(any, dm.any[0]), "ragged mask: any == definition" + tag);
        expect(sameBatchWords(anyOf(mr, c.g), dm.any[0]), "ragged mask: anyOf == definition" + tag);
        checkValues(rm.decrypt(key), want, "ragged mask" + tag);
        checkBits(any, anyw, key, "ragged mask: any" + tag);
        const UIntBatch ri = firstIndex(mr, c.g, planes);
        checkLabels(ri, dm, key, " ragged mask: firstIndex" + tag);
        checkValues(ri.decrypt(key), index, "ragged mask: firstIndex" + tag);
        // output elements 1.. hold the uniform operands' terms, so the same words as the call's
        for (unsigned j = 0; j < c.w; ++j)
            expect(sameFrom(rm.plane(j), uni.plane(j), 1), "loop words == call words" + tag);
        expect(sameFrom(any, anyu, 1), "loop any == call any" + tag);
        for (unsigned i = 0; i < planes; ++i)
            if (dm.has[i])
                expect(sameFrom(ri.plane(i), uidx.plane(i), 1), "loop index == call index" + tag);
        // ragged values: element 0 of every plane flips
        want = x.want;
        if (x.any[0] && x.index[0] == 0)
            want[0] ^= (1ull << c.w) - 1;
        const Def dv = grouped(mask, &vr, c.g, std::vector<uint64_t>(), 0);
        const UIntBatch rv = firstWhere(mask, vr, c.g);
        expect(sameWords(rv, UIntBatch::fromPlanes(dv.values)), "ragged values: words == definition" + tag);
        checkValues(rv.decrypt(key), want, "ragged values" + tag);
        expect(sameBatchWords(firstWhere(mask, vr.plane(0), c.g), dv.values[0]), "ragged values: the batch overload" + tag);
        for (unsigned j = 0; j < c.w; ++j)
            expect(sameFrom(rv.plane(j), uni.plane(j), 1), "ragged values: loop words == call words" + tag);
    }
    // an integer of ragged planes: element 0 is the complement
    for (unsigned w : {3u, 6u}) {
        const size_t count = 20;
        std::vector<uint64_t> a(count), lo(count), bit(count), len(count);
        for (size_t i = 0; i < count; ++i)
            a[i] = i % 4 == 0 ? 0 : rnd(w) >> (i % w);
        const UIntBatch x0 = UIntBatch::encrypt(key, a, w, 80 + w), xr = raggedInt(x0);
        a[0] ^= (1ull << w) - 1;
        for (size_t i = 0; i < count; ++i) {
            lo[i] = lowest(a[i]);
            bit[i] = a[i] & (~a[i] + 1);
            len[i] = length(a[i]);
        }
        const std::string tag = " ragged width=" + std::to_string(w);
        const unsigned planes = 3;
        const UIntBatch li = lowestSetIndex(xr, planes), lb = lowestSetBit(xr), bl = bitLength(xr, planes);
        checkValues(li.decrypt(key), lo, "lowestSetIndex" + tag);
        checkValues(lb.decrypt(key), bit, "lowestSetBit" + tag);
        checkValues(bl.decrypt(key), len, "bitLength" + tag);
        checkLabels(li, ofPlanes(xr, false, labelsOf(w, 0), planes), key, " lowestSetIndex" + tag);
        checkLabels(lb, ofPlanes(xr, false, labelsOf(w, 1), w), key, " lowestSetBit" + tag);
        checkLabels(bl, ofPlanes(xr, true, labelsOf(w, 2), planes), key, " bitLength" + tag);
        // elements 1.. against the call on the uniform integer
        checkLabels(li, ofPlanes(x0, false, labelsOf(w, 0), planes), key, " loop == call: lowestSetIndex" + tag, 1);
        const UIntBatch ub = lowestSetBit(x0), ul = bitLength(x0, planes);
        for (unsigned i = 0; i < w; ++i)
            expect(sameFrom(lb.plane(i), ub.plane(i), 1), "loop == call: lowestSetBit" + tag);
        for (unsigned i = 0; i < planes && (1u << i) <= w; ++i)
            expect(sameFrom(bl.plane(i), ul.plane(i), 1), "loop == call: bitLength" + tag);
    }
    return 0;
}

// Groups of 32 fresh rows at N=1247: 2^32 - 1 entries.  The size check comes first, so the call throws
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
    thrown += throws<std::invalid_argument>([&] { firstWhere(mask, vals, 32); });
    thrown += throws<std::invalid_argument>([&] { firstWhere(mask, vals.plane(0), 32); });
    thrown += throws<std::invalid_argument>([&] { anyOf(mask, 32); });
    thrown += throws<std::invalid_argument>([&] { firstIndex(mask, 32, 5); });
    thrown += throws<std::invalid_argument>([&] { firstWhere(mask, vals, 64); });       // 2^64 - 1 entries
    thrown += throws<std::invalid_argument>([&] { lowestSetIndex(wide, 5); });
    thrown += throws<std::invalid_argument>([&] { lowestSetBit(wide); });
    thrown += throws<std::invalid_argument>([&] { bitLength(wide, 6); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 8, "oversize throws (" + std::to_string(thrown) + " of 8)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    // groups, planes, counts, contexts
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { firstWhere(mask, vals, 0); });                        // groups
    thrown += throws<std::invalid_argument>([&] { firstWhere(mask, vals, 65); });
    thrown += throws<std::invalid_argument>([&] { firstWhere(mask, vals, 3); });                        // 320 % 3
    thrown += throws<std::invalid_argument>([&] { anyOf(mask, 0); });
    thrown += throws<std::invalid_argument>([&] { anyOf(mask, 7); });
    thrown += throws<std::invalid_argument>([&] { firstIndex(mask, 65, 3); });
    thrown += throws<std::invalid_argument>([&] { firstIndex(mask, 4, 0); });                           // planes
    thrown += throws<std::invalid_argument>([&] { firstIndex(mask, 4, 65); });
    thrown += throws<std::invalid_argument>([&] { lowestSetIndex(vals, 0); });
    thrown += throws<std::invalid_argument>([&] { bitLength(vals, 65); });
    thrown += throws<std::invalid_argument>([&] { firstWhere(mask, vals.slice(0, 316), 4); });          // counts
    thrown += throws<std::invalid_argument>([&] { firstWhere(mask.slice(0, 316), vals.plane(0), 4); });
    Context other(127, 8);
    SecretKey okey(other);
    thrown += throws<std::invalid_argument>([&] { firstWhere(mask, UIntBatch::encrypt(okey, std::vector<uint64_t>(count, 1), 2, 9), 4); });
    thrown += throws<std::invalid_argument>([&] { firstWhere(CiphertextBatch::encrypt(okey, randomBits(count), 9), vals.plane(1), 4); });
    expect(thrown == 14, "bad groups, planes, counts and contexts throw (" + std::to_string(thrown) + " of 14)");
    // empty batches: empty planes
    CiphertextBatch any = mask;
    const UIntBatch none = firstWhere(mask.slice(0, 0), vals.slice(0, 0), 4, &any);
    expect(none.width() == 2 && none.size() == 0 && any.size() == 0, "an empty batch gives empty planes");
    expect(anyOf(mask.slice(0, 0), 8).size() == 0, "anyOf of an empty batch");
    const UIntBatch fi = firstIndex(mask.slice(0, 0), 8, 5, &any);
    expect(fi.width() == 5 && fi.size() == 0 && any.size() == 0, "firstIndex of an empty batch");
    const UIntBatch e = vals.slice(0, 0);
    expect(lowestSetIndex(e, 3).width() == 3 && lowestSetIndex(e, 3).size() == 0 && lowestSetBit(e).width() == 2 &&
               lowestSetBit(e).size() == 0 && bitLength(e, 4).width() == 4 && bitLength(e, 4).size() == 0,
           "an empty integer gives empty planes");
    // the routes
    expect(std::string(firstRoute(8, true)) == "call" && std::string(firstRoute(1, true)) == "call" &&
               std::string(firstRoute(64, true)) == "call",
           "uniform operands: the call");
    expect(std::string(firstRoute(8, false)) == "loop" && std::string(firstRoute(0, true)) == "loop" &&
               std::string(firstRoute(65, true)) == "loop",
           "ragged operands or a group the call refuses: the loop");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 5231, "uint_first_driver", {{"words", words}, {"ragged", ragged}, {"errors", errors}});
}
