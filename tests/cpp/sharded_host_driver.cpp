// sharded_host_driver.cpp -- certFHE::ShardGroup / ShardedBatch (csgn_amd/csrc/certfhe_shard/ShardedBatch.cpp) over the
// real communicator code (csgn_amd/csrc/csgn_shard_comm.cpp) at world sizes 1 to 8 on a CPU: the two are compiled with
// the host compiler and linked with the seven base class sources, the host stub of the C ABI (capi_stub.cpp,
// capi_stub_shard.cpp), an in-process fake of the HIP and RCCL calls the communicator code makes (fake_hip_rccl.cpp)
// and oracle/csgn_oracle.c.  No HIP or RCCL library is linked; stand-alone, with its own main, so that it can be built
// with sanitizers.
//
// Every expected word, bit, count and digest is the oracle's, evaluated here by GLOBAL element index; none comes from
// another run of the code under test (that a world-W group agrees with a world-1 group is asserted on top).  Rank r
// runs on device r + 1 and the application thread sits on device 0, so a rank number used as a device number, or
// memory of one rank touched from another's thread, ends the program in the stub's device check.
//
//   sharded_host_driver compare W
//   sharded_host_driver fail W LIMIT_MS | fail_mid W LIMIT_MS | stuck W LIMIT_MS GRACE_MS
//   sharded_host_driver pool | lifetime
// LIMIT_MS bounds every call that is expected to fail: past it the program says HANG and exits 4 (the test computes it
// from the communicator's abort grace, which one failing call may have to sit out once per peer).  GRACE_MS is that
// grace: in `stuck` the peers are inside an RCCL call when the failing rank aborts them, and the call cannot return sooner.
#include "driver.h"

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "ShardedBatch.h"
#include "capi_stub.h"
#include "csgn_oracle.h"
#include "csgn_shard.h"
#include "fake_hip_rccl.h"

using namespace certFHE;
using namespace capi_stub;
using namespace fake;

#if defined(__SANITIZE_THREAD__)
#include <pthread.h>
#include <time.h>
// condition_variable::wait_for waits on the steady clock through pthread_cond_clockwait, which older ThreadSanitizer
// runtimes do not intercept: they take the mutex for held across the wait and report a double lock and races on
// everything it guards (csgn_comm_abort's grace is such a wait).  In the ThreadSanitizer build the wait goes through
// pthread_cond_timedwait, which every runtime knows, with the deadline moved to the realtime clock.
extern "C" int pthread_cond_clockwait(pthread_cond_t *cond, pthread_mutex_t *mutex, clockid_t clock, const struct timespec *deadline)
{
    struct timespec on_clock, real;
    clock_gettime(clock, &on_clock);
    clock_gettime(CLOCK_REALTIME, &real);
    long long ns = (deadline->tv_sec - on_clock.tv_sec) * 1000000000ll + (deadline->tv_nsec - on_clock.tv_nsec);
    if (ns < 0)
        ns = 0;
    ns += real.tv_sec * 1000000000ll + real.tv_nsec;
    real.tv_sec = (time_t)(ns / 1000000000ll);
    real.tv_nsec = (long)(ns % 1000000000ll);
    return pthread_cond_timedwait(cond, mutex, &real);
}
#endif

namespace {

int g_world = 1;
long g_limit_ms = 0, g_grace_ms = 0;

struct Shape {
    uint64_t n, d;
};
const Shape kShapes[] = {{1247, 16}, {64, 2}, {130, 5}};

std::vector<int> devicesOf(int world)           // rank r on device r + 1
{
    std::vector<int> v;
    for (int r = 0; r < world; ++r)
        v.push_back(r + 1);
    return v;
}

std::string tagOf(const Shape &s, int world, uint64_t count, int grouped)
{
    return "N=" + std::to_string(s.n) + " D=" + std::to_string(s.d) + " W=" + std::to_string(world) + " B=" + std::to_string(count) +
           (grouped ? " grouped" : " plain");
}

// ---- the model: a batch as the oracle has it, element after element

struct Model {
    uint64_t terms;
    std::vector<uint64_t> w;                    // count * terms * dl words
};

struct Oracle {
    uint64_t n, d, dl;
    std::vector<uint64_t> key;
    Oracle(const Context &ctx, const SecretKey &k) : n(ctx.getN()), d(k.getLength()), dl(ctx.getDefaultN()), key(k.getKey(), k.getKey() + k.getLength()) {}

    Model encrypt(const std::vector<unsigned char> &bits, uint64_t seed, uint64_t first) const
    {
        Model m{1, std::vector<uint64_t>(bits.size() * dl)};
        uint32_t k[8];
        uint64_t nonce = 0;
        csgn_oracle_rng_from_seed(seed, k, &nonce);
        if (!bits.empty())
            csgn_oracle_encrypt_keyed(n, d, key.data(), bits.size(), first, bits.data(), k, nonce, 8, m.w.data());
        return m;
    }
    Model synthetic(uint64_t count, uint64_t terms, uint64_t seed) const
    {
        Model m{terms, std::vector<uint64_t>(count * terms * dl)};
        if (!m.w.empty())
            csgn_oracle_synth_fill(seed, n, 0, m.w.size(), m.w.data());
        return m;
    }
    uint64_t count(const Model &a) const { return a.w.size() / (a.terms * dl); }
    Model mul(const Model &a, const Model &b) const
    {
        const uint64_t c = count(a);
        Model m{a.terms * b.terms, std::vector<uint64_t>(c * a.terms * b.terms * dl)};
        for (uint64_t i = 0; i < c; ++i)
            csgn_oracle_mul(dl, &a.w[i * a.terms * dl], a.terms * dl, nullptr, &b.w[i * b.terms * dl], b.terms * dl, &m.w[i * m.terms * dl], nullptr);
        return m;
    }
    Model add(const Model &a, const Model &b) const
    {
        const uint64_t c = count(a);
        Model m{a.terms + b.terms, std::vector<uint64_t>(c * (a.terms + b.terms) * dl)};
        for (uint64_t i = 0; i < c; ++i)
            csgn_oracle_add(&a.w[i * a.terms * dl], a.terms * dl, nullptr, &b.w[i * b.terms * dl], b.terms * dl, nullptr, &m.w[i * m.terms * dl], nullptr);
        return m;
    }
    Model permute(const Model &a, const Permutation &p) const     // ONE term out: the permuted first term
    {
        const uint64_t c = count(a);
        Model m{1, std::vector<uint64_t>(c * dl)};
        for (uint64_t i = 0; i < c; ++i)
            csgn_oracle_permute_ciphertext(n, p.getPermutation(), &a.w[i * a.terms * dl], a.terms * dl, nullptr, &m.w[i * dl]);
        return m;
    }
    std::vector<unsigned char> decrypt(const Model &a) const
    {
        const uint64_t c = count(a);
        std::vector<unsigned char> bits(c);
        for (uint64_t i = 0; i < c; ++i)
            bits[i] = (unsigned char)csgn_oracle_decrypt_canonical(n, d, key.data(), &a.w[i * a.terms * dl], a.terms * dl);
        return bits;
    }
    uint64_t digest(const Model &a) const { return a.w.empty() ? 0 : csgn_oracle_digest(a.w.data(), a.w.size(), 0); }
};

// every element's words through values(i), the digest, the sizes
void checkBatch(const ShardedBatch &s, const Model &m, const Oracle &o, const std::string &tag)
{
    const uint64_t count = o.count(m), per = m.terms * o.dl;
    expect(s.size() == count && s.terms() == m.terms, tag + ": size and terms");
    if (s.size() != count || s.terms() != m.terms)
        return;
    for (uint64_t i = 0; i < count; ++i)
        expect(s.values(i) == std::vector<uint64_t>(m.w.begin() + i * per, m.w.begin() + (i + 1) * per),
               tag + ": values(" + std::to_string(i) + ")");
    expect(s.digest() == o.digest(m), tag + ": digest");
}

void checkRanges(const ShardedBatch &s, int world, uint64_t count, const std::string &tag)
{
    uint64_t prev = 0;
    expect(s.shards() == world, tag + ": shards()");
    for (int r = 0; r < world; ++r) {
        const std::pair<uint64_t, uint64_t> range = s.shardRange(r);
        // ceil(r*B/W) in plain integers, not through the library
        expect(range.first == (r * count + world - 1) / world && range.second == ((r + 1) * count + world - 1) / world,
               tag + ": shardRange(" + std::to_string(r) + ")");
        expect(range.first == prev, tag + ": ranges are contiguous");
        prev = range.second;
    }
    expect(prev == count, tag + ": ranges cover the batch");
}

void checkNothingLeft(const std::string &tag)
{
    expect(stub_live_count(kDevice) == 0, tag + ": " + std::to_string(stub_live_count(kDevice)) + " device blocks left");
    expect(fake_live_comms() == 0 && fake_live_streams() == 0 && fake_live_events() == 0,
           tag + ": live communicators / streams / events: " + std::to_string(fake_live_comms()) + " / " +
               std::to_string(fake_live_streams()) + " / " + std::to_string(fake_live_events()));
}

std::vector<unsigned char> bitsA(uint64_t count)
{
    std::vector<unsigned char> v(count);
    for (uint64_t i = 0; i < count; ++i)
        v[i] = (unsigned char)((i * 7 + 1) % 3 == 0);
    return v;
}
std::vector<unsigned char> bitsB(uint64_t count)
{
    std::vector<unsigned char> v(count);
    for (uint64_t i = 0; i < count; ++i)
        v[i] = (unsigned char)((i * 5 + 2) % 2);
    return v;
}

// ---- compare

void compareOne(ShardGroup &group, ShardGroup *one, const Shape &shape, uint64_t count, int grouped)
{
    const int world = group.size();
    const std::string tag = tagOf(shape, world, count, grouped);
    Context ctx(shape.n, shape.d);
    SecretKey key(ctx);
    const Oracle o(ctx, key);
    const std::vector<unsigned char> pa = bitsA(count), pb = bitsB(count);
    group.forceGroupedBroadcast(grouped != 0);
    const uint64_t gathers0 = fake_completed("allgather"), casts0 = fake_completed("broadcast");

    const size_t mark = stub_log_size();
    ShardedBatch sa = ShardedBatch::encrypt(group, key, pa, 77, 1000), sb = ShardedBatch::encrypt(group, key, pb, 78, 5);
    {
        // a rank with nothing to encrypt is sent nothing: the key's indices and mask stay off its GPU
        const std::vector<Call> log = stub_log();
        for (size_t i = mark; i < log.size(); ++i)
            for (int r = 0; r < world; ++r)
                if (log[i].name == "csgn_memcpy_h2d" && log[i].device == r + 1)
                    expect(sa.shardRange(r).first != sa.shardRange(r).second, tag + ": key material copied to rank " + std::to_string(r) + ", whose shard is empty");
    }
    const Model ma = o.encrypt(pa, 77, 1000), mb = o.encrypt(pb, 78, 5);
    checkBatch(sa, ma, o, tag + " encrypt a");
    checkBatch(sb, mb, o, tag + " encrypt b");
    checkRanges(sa, world, count, tag);

    ShardedBatch sp = sa * sb, ss = sa + sb, sq = ss * sp;
    const Model mp = o.mul(ma, mb), ms = o.add(ma, mb), mq = o.mul(ms, mp);
    checkBatch(sp, mp, o, tag + " a*b");
    checkBatch(ss, ms, o, tag + " a+b");
    checkBatch(sq, mq, o, tag + " (a+b)*(a*b)");

    ShardedBatch sf = ShardedBatch::encryptProduct(group, key, pa, pb, 77, 78, 1000);
    checkBatch(sf, o.mul(ma, o.encrypt(pb, 78, 1000)), o, tag + " encryptProduct");

    Permutation perm(ctx);
    ShardedBatch spm = sq.applyPermutation(perm);
    checkBatch(spm, o.permute(mq, perm), o, tag + " applyPermutation");

    // bits: the oracle's decryption of the oracle's words, and the clear circuit
    const std::vector<unsigned char> dp = sp.decrypt(key), ds = ss.decrypt(key), dq = sq.decrypt(key);
    expect(dp == o.decrypt(mp) && ds == o.decrypt(ms) && dq == o.decrypt(mq), tag + " decrypt");
    for (uint64_t i = 0; i < count; ++i)
        expect(dp.size() == count && ds.size() == count && dp[i] == (pa[i] & pb[i]) && ds[i] == (pa[i] ^ pb[i]), tag + " decrypt: the clear circuit");
    expect(ss.decryptProduct(sp, key) == o.decrypt(mq), tag + " decryptProduct");
    expect(sa.decryptSum(sb, key) == o.decrypt(ms), tag + " decryptSum");
    SecretKey pkey = key.applyPermutation(perm);
    expect(sa.applyPermutation(perm).decrypt(pkey) == pa, tag + " a permuted batch under the permuted key");
    // OS entropy: the words are nobody's to predict; the bits are
    expect(ShardedBatch::encrypt(group, key, pa).decrypt(key) == pa, tag + " encrypt from OS entropy decrypts");

    const std::vector<uint64_t> cp = sp.termCounts(), cq = sq.termCounts();
    expect(cp == std::vector<uint64_t>(count, 1) && cq == std::vector<uint64_t>(count, 2), tag + " termCounts");

    // 3 x 5 terms, synthetic words at the element's global word position
    ShardedBatch y3 = ShardedBatch::synthetic(group, ctx, count, 3, 11), y5 = ShardedBatch::synthetic(group, ctx, count, 5, 12);
    const Model m3 = o.synthetic(count, 3, 11), m5 = o.synthetic(count, 5, 12);
    checkBatch(y3, m3, o, tag + " synthetic 3");
    ShardedBatch y15 = y3 * y5;
    checkBatch(y15, o.mul(m3, m5), o, tag + " synthetic 3 x 5");
    expect(y15.termCounts() == std::vector<uint64_t>(count, 15), tag + " termCounts 15");
    y15.synchronize();

    // the form of the gather that ran (none at count 0: there is nothing to exchange)
    const uint64_t gathers = fake_completed("allgather") - gathers0, casts = fake_completed("broadcast") - casts0;
    const bool equal = count % world == 0;
    if (count == 0)
        expect(gathers == 0 && casts == 0, tag + ": no collective for an empty batch");
    else if (equal && !grouped)
        expect(gathers > 0 && casts == 0, tag + ": equal shards take ncclAllGather");
    else
        expect(gathers == 0 && casts > 0, tag + ": uneven or forced shards take the grouped broadcast");

    if (one) {                                                           // on top: the same digests on a group of one
        one->forceGroupedBroadcast(grouped != 0);
        ShardedBatch a1 = ShardedBatch::encrypt(*one, key, pa, 77, 1000), b1 = ShardedBatch::encrypt(*one, key, pb, 78, 5);
        ShardedBatch q1 = (a1 + b1) * (a1 * b1);
        expect(a1.digest() == sa.digest() && q1.digest() == sq.digest() && q1.decrypt(key) == dq && q1.termCounts() == cq,
               tag + ": equal to the world-1 run");
    }
    expect(group.healthy(), tag + ": healthy");
}

int compare()
{
    const int world = g_world;
    const std::vector<int> devs = devicesOf(world);
    fake_hip_device_count(world + 1);
    expect(csgn_init(0) == CSGN_OK, "application thread on device 0");
    {
        ShardGroup group(devs);
        expect(stub_device() == 0, "making a group leaves the caller's current device alone");
        expect(group.size() == world && group.device(world - 1) == world, "group size and devices");
        expect(group.collective().find("RCCL 2.") == 0, "collective(): " + group.collective());
        std::unique_ptr<ShardGroup> one(world > 1 ? new ShardGroup(std::vector<int>(1, 1)) : nullptr);
        const uint64_t w = (uint64_t)world;
        std::vector<uint64_t> counts = {0, 1, 2, w - 1, w, w + 1, 2 * w + 1, 61};
        for (const Shape &shape : kShapes)
            for (uint64_t count : counts)
                for (int grouped = 0; grouped < 2; ++grouped)
                    compareOne(group, one.get(), shape, count, grouped);

        // knobs are per host thread: setTuning reaches every worker, each on its own device; a typo is no rank failure
        const size_t mark = stub_log_size();
        group.setTuning("mul_flat", -1);
        const std::vector<Call> log = stub_log();
        std::vector<int> seen;
        for (size_t i = mark; i < log.size(); ++i)
            if (log[i].name == "csgn_set_tuning" && log[i].status == CSGN_OK && (int)log[i].bytes == -1)
                seen.push_back(log[i].device);
        std::sort(seen.begin(), seen.end());
        expect(seen == devs, "setTuning: one csgn_set_tuning on every rank's device");
        expect(throws<std::invalid_argument>([&] { group.setTuning("no_such_knob", 1); }) && group.healthy(),
               "setTuning: an unknown knob is invalid_argument and the group lives");
    }
    checkNothingLeft("compare");
    return 0;
}

// ---- calls that must fail, under a watchdog

// f() must throw; -> what() and the milliseconds it took.  Past g_limit_ms the program ends: a hang is a failure here,
// not something the test's patience finds.
std::string mustThrow(const std::function<void()> &f, const std::string &tag, long *took_ms = nullptr)
{
    std::mutex m;
    std::condition_variable cv;
    bool over = false;
    std::thread dog([&] {
        std::unique_lock<std::mutex> lk(m);
        if (!cv.wait_for(lk, std::chrono::milliseconds(g_limit_ms), [&] { return over; })) {
            printf("HANG %s: no return within %ld ms\n", tag.c_str(), g_limit_ms);
            fflush(stdout);
            _Exit(4);
        }
    });
    const auto t0 = std::chrono::steady_clock::now();
    std::string what;
    bool threw = false;
    try {
        f();
    } catch (const std::exception &e) {
        threw = true;
        what = e.what();
    }
    const long ms = (long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
    {
        std::lock_guard<std::mutex> g(m);
        over = true;
    }
    cv.notify_all();
    dog.join();
    printf("%s: %ld ms: %s\n", tag.c_str(), ms, threw ? what.c_str() : "(no exception)");
    expect(threw, tag + ": the call throws");
    if (took_ms)
        *took_ms = ms;
    return what;
}

bool has(const std::string &text, const std::string &part) { return text.find(part) != std::string::npos; }

// Holding one rank back.  An injected failure throws as soon as the rank's task starts, long before its peers reach
// the collective, and then nobody is blocked when the abort comes.  So the failing rank's worker is kept busy first: a
// second application thread calls synchronize(), whose csgn_stream_sync on that rank's device stays in the stream hook
// below until every peer has a collective registered that cannot run (or LIMIT_MS is over); the failing call's task
// sits behind it in that rank's queue.
void (*g_fake_hook)(void *) = nullptr;
std::atomic<int> g_hold_device{-1}, g_hold_peers{0};
std::atomic<bool> g_holding{false};

void holdingHook(void *stream)
{
    g_fake_hook(stream);
    if (stub_device() != g_hold_device.load())
        return;
    g_holding.store(true);
    const auto t0 = std::chrono::steady_clock::now();
    while ((int)fake_pending_ranks() < g_hold_peers.load() && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(g_limit_ms))
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    g_hold_device.store(-1);
}

// injectFailure(r) before termCounts() and before decrypt(), for every rank r: the peers are in the gather / barrier
// that r never joins
void failEveryRank(bool inside)
{
    const int world = g_world;
    const std::vector<int> devs = devicesOf(world);
    fake_hip_device_count(world + 1);
    fake_rccl_block_inside(inside);
    if (!g_fake_hook) {
        g_fake_hook = stub_stream_hook;
        stub_stream_hook = holdingHook;
    }
    expect(csgn_init(0) == CSGN_OK, "application thread on device 0");
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const std::vector<unsigned char> bits = bitsA(2 * (uint64_t)world + 1);
    for (int r = 0; r < world; ++r)
        for (int phase = 0; phase < 2; ++phase) {
            const std::string tag = std::string(inside ? "stuck" : "fail") + " W=" + std::to_string(world) + " rank " + std::to_string(r) +
                                    (phase ? " decrypt" : " termCounts");
            {
                ShardGroup group(devs);
                ShardedBatch a = ShardedBatch::encrypt(group, key, bits, 5), b = a * a;
                b.synchronize();
                const uint64_t cancelled = fake_cancelled();
                g_holding.store(false);
                g_hold_peers.store(world - 1);
                g_hold_device.store(r + 1);
                std::thread other([&] {
                    try {
                        a.synchronize();                   // (throws once the group is dead: every call does)
                    } catch (const std::exception &) {
                    }
                });
                while (!g_holding.load())
                    std::this_thread::sleep_for(std::chrono::microseconds(100));
                group.injectFailure(r);                    // rank r's next task: the one queued behind the held synchronize
                long ms = 0;
                const std::string what = mustThrow([&] { phase ? (void)b.decrypt(key) : (void)b.termCounts(); }, tag, &ms);
                other.join();
                expect(has(what, "rank " + std::to_string(r) + " (device " + std::to_string(r + 1) + ")") && has(what, "injected failure"),
                       tag + ": names the rank and its error: " + what);
                // every peer had registered its gather when the abort came, and the abort cancelled it
                expect(fake_cancelled() - cancelled >= (uint64_t)(world - 1), tag + ": the abort cancelled the peers' pending collectives");
                // every peer was inside RCCL, so the first abort of a peer sat out the whole grace (the later ones overlap:
                // a peer that is thrown out runs abortAll itself, next to the failing rank's)
                if (inside && world > 1)
                    expect(ms >= g_grace_ms * 9 / 10, tag + ": returned before a peer's grace was over");
                expect(!group.healthy(), tag + ": the group is dead");
                const auto t0 = std::chrono::steady_clock::now();
                expect(has(mustThrow([&] { (void)(a * a); }, tag + " next call"), "dead"), tag + ": the next call says dead");
                expect(std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(g_grace_ms ? g_grace_ms : g_limit_ms),
                       tag + ": the next call fails at once");
            }
            checkNothingLeft(tag);
        }
}

int fail()
{
    failEveryRank(false);
    return 0;
}

int stuck()
{
    failEveryRank(true);
    // a rank that joins late, a small timeout: the barrier of the ranks that wait gives up
    fake_rccl_block_inside(false);
    const int world = g_world;
    const std::vector<int> devs = devicesOf(world);
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const std::string tag = "late W=" + std::to_string(world);
    {
        ShardGroup group(devs);
        ShardedBatch a = ShardedBatch::encrypt(group, key, bitsA(2 * (uint64_t)world + 1), 5);
        group.setTimeoutMs(50);
        fake_rccl_delay(world - 1, (int)(g_grace_ms / 2));
        const std::string what = mustThrow([&] { (void)a.decrypt(key); }, tag);
        expect(has(what, "csgn_comm_barrier failed [" + std::to_string(CSGN_ERR_TIMEOUT) + "]") && has(what, "waited") && has(what, "ms for its peers"),
               tag + ": the barrier's timeout is the group's error: " + what);
        expect(!group.healthy(), tag + ": the group is dead");
    }
    checkNothingLeft(tag);
    return 0;
}

// one rank fails in the middle of an operation, after it took its work block
int failMid()
{
    const int world = g_world;
    const std::vector<int> devs = devicesOf(world);
    fake_hip_device_count(world + 1);
    expect(csgn_init(0) == CSGN_OK, "application thread on device 0");
    Context ctx(130, 5);
    SecretKey key(ctx);
    const std::vector<unsigned char> bits = bitsA(2 * (uint64_t)world + 1);
    const char *entries[] = {"csgn_decrypt_uniform", "csgn_encrypt_keyed", "csgn_digest"};
    for (int e = 0; e < 3; ++e) {
        const std::string entry = entries[e], tag = "fail_mid W=" + std::to_string(world) + " " + entry;
        {
            ShardGroup group(devs);
            ShardedBatch a = ShardedBatch::encrypt(group, key, bits, 5);
            a.synchronize();
            stub_fail(entries[e], world > 1 ? 1 : 0, 1, CSGN_ERR_HIP);          // the second rank to get there
            const std::string what = mustThrow([&] {
                if (e == 0)
                    (void)a.decrypt(key);
                else if (e == 1)
                    (void)ShardedBatch::encrypt(group, key, bits, 6);
                else
                    (void)a.termCounts();
            }, tag);
            stub_fail_clear();
            expect(has(what, entry + " failed [" + std::to_string(CSGN_ERR_HIP) + "]") && has(what, "stub: " + entry + " refused") && has(what, "rank "),
                   tag + ": the stub's error text reaches the caller: " + what);
            expect(!group.healthy(), tag + ": the group is dead");
        }
        checkNothingLeft(tag);
    }
    return 0;
}

// ---- the per-rank block pools and the wipe of the staging block

// does any live device block of the group's devices hold `words` (at any 8-byte offset)?
bool liveBlocksHold(const std::vector<int> &devices, const std::vector<uint64_t> &words)
{
    for (const Alloc &a : stub_live()) {
        bool ours = false;
        for (int d : devices)
            ours = ours || a.device == d;
        if (!ours || a.kind != kDevice || a.bytes < words.size() * 8)
            continue;
        const unsigned char *p = static_cast<const unsigned char *>(a.ptr);
        for (size_t off = 0; off + words.size() * 8 <= a.bytes; off += 8)
            if (memcmp(p + off, words.data(), words.size() * 8) == 0)
                return true;
    }
    return false;
}

int pool()
{
    const int world = 3;
    const std::vector<int> devs = devicesOf(world);
    fake_hip_device_count(world + 1);
    expect(csgn_init(0) == CSGN_OK, "application thread on device 0");
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const Oracle o(ctx, key);
    const std::vector<unsigned char> pa = bitsA(7), pb = bitsB(7);
    std::vector<uint64_t> mask(o.dl, 0);
    csgn_oracle_key_mask(o.n, o.key.data(), o.d, mask.data());
    {
        ShardGroup group(devs);
        // an empty pool and no memory: the operation fails (on a group of its own: a failure kills the group)
        {
            ShardGroup poor(devs);
            stub_fail("csgn_malloc", 0, 1, CSGN_ERR_HIP);
            const std::string what = [&] {
                try {
                    (void)ShardedBatch::synthetic(poor, ctx, 7, 1, 3);
                } catch (const std::exception &e) {
                    return std::string(e.what());
                }
                return std::string();
            }();
            stub_fail_clear();
            expect(has(what, "csgn_malloc failed") && !poor.healthy(), "pool: out of memory with an empty pool throws: " + what);
        }
        ShardedBatch a = ShardedBatch::encrypt(group, key, pa, 77, 0), b = ShardedBatch::encrypt(group, key, pb, 78, 0);
        expect(!liveBlocksHold(devs, o.key) && !liveBlocksHold(devs, mask), "pool: no key indices or mask in device memory after encrypt");
        const Model ma = o.encrypt(pa, 77, 0), mb = o.encrypt(pb, 78, 0);
        {
            ShardedBatch p = a * b;
            p.synchronize();
        }
        a.synchronize();                                   // the give-backs of p are behind this in every rank's queue
        {
            ShardedBatch p = a * b;
            checkBatch(p, o.mul(ma, mb), o, "pool: second product");
            expect(p.decrypt(key) == o.decrypt(o.mul(ma, mb)), "pool: decrypt");
            expect(!liveBlocksHold(devs, o.key) && !liveBlocksHold(devs, mask), "pool: no key indices or mask in device memory after decrypt");
        }
        a.synchronize();
        {
            const uint64_t before = stub_calls("csgn_malloc");
            ShardedBatch p = a * b;
            p.synchronize();
            expect(stub_calls("csgn_malloc") == before, "pool: a product of a shape the pool holds makes no csgn_malloc");
        }
        a.synchronize();
        // memory refused once with blocks in the pool: that rank drops its pool and tries again
        const uint64_t frees = stub_calls("csgn_free");
        stub_fail("csgn_malloc", 0, 1, CSGN_ERR_HIP);
        ShardedBatch s = a + b;                            // two terms: no block of that size in any pool
        stub_fail_clear();
        expect(stub_calls("csgn_free") > frees, "pool: the refused rank dropped its pool");
        checkBatch(s, o.add(ma, mb), o, "pool: the sum after the retry");
        expect(group.healthy(), "pool: healthy");
    }
    checkNothingLeft("pool");
    return 0;
}

// ---- who outlives whom

int lifetime()
{
    const int world = 3;
    const std::vector<int> devs = devicesOf(world);
    fake_hip_device_count(2 * world + 1);
    expect(csgn_init(0) == CSGN_OK, "application thread on device 0");
    Context ctx(130, 5);
    SecretKey key(ctx);
    const Oracle o(ctx, key);
    const std::vector<unsigned char> pa = bitsA(7), pb = bitsB(7);
    const Model ma = o.encrypt(pa, 77, 0), mb = o.encrypt(pb, 78, 0);
    {
        // the batch outlives the ShardGroup object; the last batch dies with its products' give-backs still queued
        std::unique_ptr<ShardedBatch> a, b;
        {
            ShardGroup group(devs);
            a.reset(new ShardedBatch(ShardedBatch::encrypt(group, key, pa, 77, 0)));
            b.reset(new ShardedBatch(ShardedBatch::encrypt(group, key, pb, 78, 0)));
        }
        checkBatch(*a * *b, o.mul(ma, mb), o, "lifetime: a product after the group object is gone");
        expect(a->decrypt(key) == pa, "lifetime: decrypt after the group object is gone");
        expect(throws<std::out_of_range>([&] { (void)a->values(7); }), "lifetime: values(count) is out_of_range");
        {
            std::vector<int> other;
            for (int r = 0; r < world; ++r)
                other.push_back(world + 1 + r);
            ShardGroup second(other);
            ShardedBatch c = ShardedBatch::encrypt(second, key, pb, 78, 0);
            expect(throws<std::invalid_argument>([&] { (void)(*a * c); }) && throws<std::invalid_argument>([&] { (void)(*a + c); }) &&
                       throws<std::invalid_argument>([&] { (void)a->decryptSum(c, key); }),
                   "lifetime: operands of two groups are invalid_argument");
        }
        for (int i = 0; i < 4; ++i)
            (void)(*a * *b);                               // temporaries: four give-backs per rank, nothing waits for them
        b.reset();
        a.reset();                                         // the last owner of the group
    }
    checkNothingLeft("lifetime: batches after their group");
    {
        // two application threads, one after the other, on one group
        ShardGroup group(devs);
        std::unique_ptr<ShardedBatch> a, p;
        uint64_t digest = 0;
        std::thread first([&] {
            a.reset(new ShardedBatch(ShardedBatch::encrypt(group, key, pa, 77, 0)));
            p.reset(new ShardedBatch(*a * ShardedBatch::encrypt(group, key, pb, 78, 0)));
        });
        first.join();
        std::vector<unsigned char> bits;
        std::thread second([&] {
            digest = p->digest();
            bits = p->decrypt(key);
            p.reset();
            a.reset();
        });
        second.join();
        expect(digest == o.digest(o.mul(ma, mb)) && bits == o.decrypt(o.mul(ma, mb)), "lifetime: a second application thread reads the first one's batch");
    }
    checkNothingLeft("lifetime: two application threads");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    const bool sized = mode == "compare" || mode == "fail" || mode == "fail_mid" || mode == "stuck";
    const bool timed = mode == "fail" || mode == "fail_mid" || mode == "stuck";
    g_world = argc > 2 ? atoi(argv[2]) : 0;
    g_limit_ms = argc > 3 ? atol(argv[3]) : 0;
    g_grace_ms = argc > 4 ? atol(argv[4]) : 0;
    if ((sized && (g_world < 1 || g_world > 8)) || (timed && g_limit_ms <= 0) || (mode == "stuck" && g_grace_ms <= 0))
        argc = 1;                                          // -> the usage, exit 2
    return runModes(argc, argv, 20260101u, "sharded_host_driver (compare W | fail W LIMIT_MS | fail_mid W LIMIT_MS | stuck W LIMIT_MS GRACE_MS | pool | lifetime)",
                    {{"compare", compare}, {"fail", fail}, {"fail_mid", failMid}, {"stuck", stuck}, {"pool", pool}, {"lifetime", lifetime}});
}
