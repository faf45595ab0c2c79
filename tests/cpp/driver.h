// driver.h -- what the operation drivers in tests/cpp share (header-only C++11; each driver is one translation unit):
// the mismatch count, word-for-word comparisons, the check of decrypted values, the rand() draws the inputs are made
// of, and runModes(), the whole of every driver's main().
#ifndef CSGN_TESTS_DRIVER_H
#define CSGN_TESTS_DRIVER_H

#include "certFHE.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <initializer_list>
#include <string>
#include <vector>

namespace {

int fails = 0;

// counts a mismatch; the first ten are printed
inline void expect(bool ok, const std::string &what)
{
    if (!ok && fails++ < 10)
        printf("MISMATCH %s\n", what.c_str());
}

inline bool sameWords(const certFHE::Ciphertext &x, const certFHE::Ciphertext &y)
{
    return x.getLen() == y.getLen() && (x.getLen() == 0 || memcmp(x.getValues(), y.getValues(), x.getLen() * 8) == 0);
}

inline bool sameBatchWords(const certFHE::CiphertextBatch &x, const certFHE::CiphertextBatch &y)
{
    if (x.size() != y.size())
        return false;
    for (uint64_t i = 0; i < x.size(); ++i)
        if (!sameWords(x.at(i), y.at(i)))
            return false;
    return true;
}

inline bool sameWords(const certFHE::UIntBatch &x, const certFHE::UIntBatch &y)
{
    if (x.width() != y.width())
        return false;
    for (unsigned j = 0; j < x.width(); ++j)
        if (!sameBatchWords(x.plane(j), y.plane(j)))
            return false;
    return true;
}

// one mismatch for the first element that differs, named with both values
inline void checkValues(const std::vector<uint64_t> &got, const std::vector<uint64_t> &want, const std::string &tag)
{
    if (got.size() != want.size()) {
        expect(false, tag + ": " + std::to_string(got.size()) + " values, " + std::to_string(want.size()) + " wanted");
        return;
    }
    for (size_t i = 0; i < want.size(); ++i)
        if (got[i] != want[i]) {
            expect(false, tag + " element " + std::to_string(i) + ": " + std::to_string(got[i]) + " != " +
                              std::to_string(want[i]));
            return;
        }
}

// one rand() draw a bit
inline std::vector<unsigned char> randomBits(size_t n)
{
    std::vector<unsigned char> v(n);
    for (size_t i = 0; i < n; ++i)
        v[i] = (unsigned char)(rand() & 1);
    return v;
}

// the low w bits (w <= 64) of two rand() draws
inline uint64_t rnd(unsigned w)
{
    return (((uint64_t)rand() << 31) ^ (uint64_t)rand()) & (w == 64 ? ~0ull : (1ull << w) - 1);
}

// f() throws an E; any other exception propagates
template <typename E, typename F>
bool throws(F f)
{
    try {
        f();
    } catch (const E &) {
        return true;
    }
    return false;
}

struct Mode {
    const char *name;
    int (*run)();
};

// srand(seed), then the mode argv[1] names.  Prints "<mode> ok" and returns 0; "N mismatches" or "EXCEPTION <what>"
// and returns 1; the usage on stderr and returns 2 for a mode not in the list.
inline int runModes(int argc, char **argv, unsigned seed, const char *program, std::initializer_list<Mode> modes)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    srand(seed);
    const Mode *chosen = nullptr;
    std::string usage;
    for (const Mode &m : modes) {
        if (mode == m.name)
            chosen = &m;
        usage += (usage.empty() ? "" : "|") + std::string(m.name);
    }
    if (!chosen) {
        fprintf(stderr, "usage: %s %s\n", program, usage.c_str());
        return 2;
    }
    try {
        chosen->run();
    } catch (const std::exception &e) {
        printf("EXCEPTION %s\n", e.what());
        return 1;
    }
    if (fails) {
        printf("%d mismatches\n", fails);
        return 1;
    }
    printf("%s ok\n", mode.c_str());
    return 0;
}

} // namespace

#endif
