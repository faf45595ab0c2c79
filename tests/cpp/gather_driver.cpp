// gather_driver.cpp -- user-style C++ over the data movement of include/certfhe/Batch.h and UInt.h
// (tests/test_gather_cpp.py builds and runs it).
//   gather_driver move    gather, slice, broadcast and concat of uniform and of compacted (ragged) batches and of integers:
//                         every element's words == the source element's, decryptions == the moved plaintext
//   gather_driver query   one encrypted 4-bit query against an encrypted table of 2^12 integers:
//                         equalTo(db, q.broadcast(n)) decrypts to db[i] == q, and its words == equalTo(db, q') where q'
//                         is built from n per-element copies through pack()
//   gather_driver throws  bad indices, ranges and shapes throw std::out_of_range / std::invalid_argument
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include <stdexcept>

using namespace certFHE;

namespace {

// out[e] is a copy of src[from[e]], word for word
void expectMoved(const CiphertextBatch &out, const CiphertextBatch &src, const std::vector<uint64_t> &from,
                 const std::string &what)
{
    expect(out.size() == from.size(), what + ": size");
    if (out.size() != from.size())
        return;
    bool same = true;
    for (uint64_t e = 0; e < from.size() && same; ++e)
        same = out.termsOf(e) == src.termsOf(from[e]) && sameWords(out.at(e), src.at(from[e]));
    expect(same, what + ": words");
}

std::vector<uint64_t> randomIndices(size_t n, uint64_t below)
{
    std::vector<uint64_t> v(n);
    for (auto &x : v)
        x = (uint64_t)rand() % below;
    return v;
}

void checkMovement(const SecretKey &key, const CiphertextBatch &src, const std::vector<unsigned char> &plain,
                   const std::string &tag)
{
    const uint64_t n = src.size();
    std::vector<uint64_t> idx = randomIndices(2 * n + 3, n);
    idx[0] = n - 1;
    const CiphertextBatch g = src.gather(idx);
    expect(g.uniform() == src.uniform(), tag + " gather keeps the layout");
    expectMoved(g, src, idx, tag + " gather");
    std::vector<unsigned char> want(idx.size());
    for (size_t e = 0; e < idx.size(); ++e)
        want[e] = plain[idx[e]];
    expect(g.decrypt(key) == want, tag + " gather decrypts");
    expect(src.gather({}).size() == 0, tag + " empty gather");

    const uint64_t b = n / 3, e = n - 2;
    const CiphertextBatch s = src.slice(b, e);
    std::vector<uint64_t> range;
    for (uint64_t i = b; i < e; ++i)
        range.push_back(i);
    expectMoved(s, src, range, tag + " slice");
    expect(s.decrypt(key) == std::vector<unsigned char>(plain.begin() + b, plain.begin() + e), tag + " slice decrypts");
    expect(src.slice(n, n).size() == 0, tag + " empty slice");

    const CiphertextBatch one = src.slice(2, 3), bc = one.broadcast(129);
    expectMoved(bc, src, std::vector<uint64_t>(129, 2), tag + " broadcast");

    const CiphertextBatch c = CiphertextBatch::concat({src.slice(0, b), src.slice(b, b), src.slice(b, n)});
    std::vector<uint64_t> all;
    for (uint64_t i = 0; i < n; ++i)
        all.push_back(i);
    expectMoved(c, src, all, tag + " concat of its slices");
    expect(c.decrypt(key) == plain, tag + " concat decrypts");
}

int move()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const size_t count = 300;
    const std::vector<unsigned char> bits = randomBits(count);
    const CiphertextBatch a = CiphertextBatch::encrypt(key, bits, 5);
    checkMovement(key, a, bits, "uniform t=1");
    const CiphertextBatch a3 = a + a * a;                          // 2 terms, Dec = a ^ a = 0
    checkMovement(key, a3, std::vector<unsigned char>(count, 0), "uniform t=2");

    // a compacted (ragged) batch: element i holds a, plus ONE and ZERO where x[i] = 1 (3 terms, the bit flipped);
    // concatenated with a part of 0-term elements
    std::vector<unsigned char> x = randomBits(count), none(count, 0), flipped(count);
    const CiphertextBatch r = addPlain(addPlain(a, x), none).compact();
    expect(!r.uniform(), "compact() gave a ragged batch");
    for (size_t i = 0; i < count; ++i)
        flipped[i] = bits[i] ^ x[i];
    checkMovement(key, r, flipped, "ragged");
    const CiphertextBatch zero = (a.slice(0, 40) + a.slice(0, 40)).compact();   // every term cancels: 0 terms
    const CiphertextBatch rz = CiphertextBatch::concat({r, zero, r.slice(0, 10)});
    std::vector<unsigned char> pz = flipped;
    pz.insert(pz.end(), 40, 0);
    pz.insert(pz.end(), flipped.begin(), flipped.begin() + 10);
    expect(!rz.uniform() && rz.size() == count + 50 && rz.termsOf(count) == 0, "concat with 0-term elements");
    checkMovement(key, rz, pz, "ragged with empty elements");

    // integers: uniform planes go through one csgn_gather_planes launch, ragged planes element by element
    std::vector<uint64_t> v(count);
    for (auto &y : v)
        y = (uint64_t)rand() & 255;
    const UIntBatch u = UIntBatch::encrypt(key, v, 8, 9);
    std::vector<uint64_t> idx = randomIndices(500, count);
    const UIntBatch ug = u.gather(idx);
    std::vector<uint64_t> want(idx.size());
    for (size_t e = 0; e < idx.size(); ++e)
        want[e] = v[idx[e]];
    expect(ug.decrypt(key) == want, "UIntBatch gather decrypts");
    for (unsigned j = 0; j < 8; ++j)
        expectMoved(ug.plane(j), u.plane(j), idx, "UIntBatch gather plane " + std::to_string(j));
    const UIntBatch ub = u.slice(7, 8).broadcast(64);
    expect(ub.decrypt(key) == std::vector<uint64_t>(64, v[7]), "UIntBatch broadcast decrypts");
    const UIntBatch uc = UIntBatch::concat({u.slice(100, count), u.slice(0, 100)});
    std::vector<uint64_t> rot(v.begin() + 100, v.end());
    rot.insert(rot.end(), v.begin(), v.begin() + 100);
    expect(uc.decrypt(key) == rot, "UIntBatch concat decrypts");
    std::vector<CiphertextBatch> pr;
    for (unsigned j = 0; j < 8; ++j)
        pr.push_back(addPlain(addPlain(u.plane(j), x), none).compact());
    const UIntBatch ur = UIntBatch::fromPlanes(pr);
    std::vector<uint64_t> wr(idx.size());
    for (size_t e = 0; e < idx.size(); ++e)
        wr[e] = x[idx[e]] ? v[idx[e]] ^ 255 : v[idx[e]];
    expect(ur.gather(idx).decrypt(key) == wr, "UIntBatch gather of ragged planes decrypts");
    return 0;
}

int query()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const size_t n = 1u << 12;
    std::vector<uint64_t> table(n);
    for (auto &y : table)
        y = (uint64_t)rand() & 15;
    const uint64_t qv = table[1234];
    const UIntBatch db = UIntBatch::encrypt(key, table, 4, 21);
    const UIntBatch q = UIntBatch::encrypt(key, std::vector<uint64_t>(1, qv), 4, 22);
    const CiphertextBatch eq = equalTo(db, q.broadcast(db.size()));
    std::vector<unsigned char> want(n);
    for (size_t i = 0; i < n; ++i)
        want[i] = table[i] == qv;
    expect(eq.decrypt(key) == want, "equalTo(db, q.broadcast(n)) decrypts");
    // today's route: n per-element copies of every plane through pack()
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < 4; ++j)
        planes.push_back(CiphertextBatch::pack(std::vector<Ciphertext>(n, q.plane(j).at(0))));
    const CiphertextBatch eq2 = equalTo(db, UIntBatch::fromPlanes(planes));
    std::vector<uint64_t> all(n);
    for (size_t i = 0; i < n; ++i)
        all[i] = i;
    expectMoved(eq, eq2, all, "equalTo words == the pack() route's");
    return 0;
}

int throwsMode()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const CiphertextBatch a = CiphertextBatch::encrypt(key, randomBits(10), 3);
    std::vector<uint64_t> big(1u << 22, 0);
    big.back() = 10;
    expect(throws<std::out_of_range>([&] { a.gather(big); }), "gather: index == size");
    expect(throws<std::out_of_range>([&] { a.gather({0, 1ull << 40}); }), "gather: huge index");
    expect(throws<std::out_of_range>([&] { a.slice(5, 3); }), "slice: begin > end");
    expect(throws<std::out_of_range>([&] { a.slice(0, 11); }), "slice: end > size");
    expect(throws<std::invalid_argument>([&] { a.broadcast(5); }), "broadcast of 10 elements");
    expect(throws<std::invalid_argument>([&] { a.slice(0, 0).broadcast(5); }), "broadcast of 0 elements");
    expect(throws<std::invalid_argument>([&] { CiphertextBatch::concat({}); }), "concat of nothing");
    Context other(1000, 16);
    SecretKey key2(other);
    const CiphertextBatch b = CiphertextBatch::encrypt(key2, randomBits(4), 3);
    expect(throws<std::invalid_argument>([&] { CiphertextBatch::concat({a, b}); }), "concat across contexts");
    const UIntBatch u = UIntBatch::encrypt(key, std::vector<uint64_t>(6, 3), 4, 1);
    expect(throws<std::out_of_range>([&] { u.gather({6}); }), "UIntBatch gather");
    expect(throws<std::out_of_range>([&] { u.slice(2, 7); }), "UIntBatch slice");
    expect(throws<std::invalid_argument>([&] { u.broadcast(3); }), "UIntBatch broadcast");
    expect(throws<std::invalid_argument>([&] { UIntBatch::concat({}); }), "UIntBatch concat of nothing");
    const UIntBatch w = UIntBatch::encrypt(key, std::vector<uint64_t>(6, 3), 3, 1);
    expect(throws<std::invalid_argument>([&] { UIntBatch::concat({u, w}); }), "UIntBatch concat of widths 4 and 3");
    expect(a.decrypt(key).size() == 10, "the source survives");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4711, "gather_driver", {{"move", move}, {"query", query}, {"throws", throwsMode}});
}
