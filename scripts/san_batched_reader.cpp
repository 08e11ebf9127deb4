// san_batched_reader.cpp — br::batched_read (thesia_amd/csrc/batched_reader.h) under AddressSanitizer and UBSan: the fake readers and
// managers of tests/emu/emu_batched_reader.cpp (included here) through fixed and random batches.  The caller's arrays have exactly
// the sizes the ABI states (n requests, n infos, cap output bytes), so a read or write past them is reported; every call is also
// checked for what tests/test_batched_reader_host.py asserts of the protocol.  Not a pytest test and never loaded into python.
// From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined scripts/san_batched_reader.cpp
//       -o build/san_batched_reader && build/san_batched_reader   (one line)
#include <cstdlib>
#include <memory>
#include <random>

#include "../tests/emu/emu_batched_reader.cpp"

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            std::exit(2);                                                             \
        }                                                                             \
    } while (0)

static std::mt19937_64 rng(20261021);
static uint64_t r(uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo); }  // [lo, hi)

static size_t calls = 0, refused = 0, short_buffers = 0, failed_runs = 0;

static void one_call(int manager, int reader, int flags, uint64_t fit_limit, const std::vector<emu::Request> &reqs, size_t cap) {
    const size_t n = reqs.size();
    // exactly-sized heap arrays (n == 0: none at all, the ABI allows NULL)
    std::unique_ptr<uint64_t[]> rq(n ? new uint64_t[3 * n] : nullptr), info(n ? new uint64_t[6 * n] : nullptr);
    std::unique_ptr<uint8_t[]> out(cap ? new uint8_t[cap] : nullptr);
    for (size_t i = 0; i < n; i++) {
        rq[3 * i] = reqs[i].id;
        rq[3 * i + 1] = reqs[i].length;
        rq[3 * i + 2] = reqs[i].fault;
    }
    for (size_t i = 0; i < 6 * n; i++) info[i] = 0xDEAD;
    if (cap) std::memset(out.get(), 0xA5, cap);
    uint64_t len = 0xBEEF;
    char msg[512];
    std::vector<uint64_t> log(64 + 16 * n);
    size_t log_len = 0;
    const int rc = emu_batched_reader(manager, reader, flags, fit_limit, rq.get(), n, out.get(), cap, info.get(), &len, msg, sizeof msg,
                                      log.data(), log.size(), &log_len);
    calls++;
    EXPECT(log_len <= log.size());
    size_t first_fault = n, total = 0, end = 0;  // what the protocol must report
    for (size_t i = 0; i < n && first_fault == n; i++)
        if (reqs[i].id >= 100 || reqs[i].fault) first_fault = i;
    std::vector<size_t> at(n);
    for (size_t i = 0; i < n; i++) {
        at[i] = total;
        end = total + reqs[i].length;
        total = reader == 0 ? (end + 63) / 64 * 64 : end;
    }
    if (n) total = end;
    auto untouched = [&] {
        for (size_t i = 0; i < cap; i++)
            if (out[i] != 0xA5) return false;
        return true;
    };
    if (manager == 2) {
        EXPECT(rc == TH_ERR_INVALID_ARG && len == 0xBEEF && untouched());
        return;
    }
    if (n == 0) {
        EXPECT(rc == TH_OK && len == 0 && log_len == 0);
        return;
    }
    if (first_fault < n) {
        EXPECT(rc == (reqs[first_fault].id >= 100 ? TH_ERR_NOT_FOUND : (int)reqs[first_fault].fault) && len == 0 && untouched());
        for (size_t i = 0; i < 6 * n; i++) EXPECT(info[i] == 0xDEAD);
        refused++;
        return;
    }
    if (manager == 0 && n > fit_limit) {
        EXPECT(rc == TH_ERR_INVALID_ARG && len == 0 && untouched() && info[0] == 0xDEAD);
        refused++;
        return;
    }
    EXPECT(len == total);
    for (size_t i = 0; i < n; i++) EXPECT(info[6 * i] == at[i] && info[6 * i + 1] == reqs[i].length && info[6 * i + (reader == 0 ? 4 : 3)] == (reader == 0 ? 42u : 41u));
    if (cap < total || !out) {  // (a NULL out is a short buffer, even of nothing)
        EXPECT(rc == TH_ERR_BUFFER_TOO_SMALL && untouched());
        for (size_t i = 0; i < n; i++) EXPECT(info[6 * i + 5] == 0);
        short_buffers++;
        return;
    }
    if (flags & emu::FAIL_RUN) {
        bool any = manager == 0;  // two owners: slot 1 fails if it has a request
        for (size_t i = 0; i < n; i++) any = any || reqs[i].id % 2 == 0;
        EXPECT(rc == (any ? TH_ERR_HIP : TH_OK));
        if (any) {
            for (size_t i = 0; i < n; i++) EXPECT(info[6 * i + 5] == 0);
            failed_runs++;
            return;
        }
    }
    EXPECT(rc == TH_OK);
    std::vector<uint8_t> want(cap, 0xA5);
    for (size_t i = 0; i < n; i++) std::memset(want.data() + at[i], (int)(reqs[i].id & 255), (size_t)reqs[i].length);
    EXPECT(cap == 0 || std::memcmp(want.data(), out.get(), cap) == 0);
    for (size_t i = 0; i < n; i++) EXPECT(info[6 * i + 5] == (reader == 0 ? 0 : 1000 + reqs[i].id));
}

int main() {
    for (int manager = 0; manager < 3; manager++)
        for (int reader = 0; reader < 2; reader++) {
            one_call(manager, reader, 0, SIZE_MAX, {}, 0);
            one_call(manager, reader, 0, SIZE_MAX, {{1, 10, 0}, {2, 70, 0}, {3, 5, 0}}, 300);
            one_call(manager, reader, 0, SIZE_MAX, {{1, 10, 0}, {2, 70, 0}, {3, 5, 0}}, 84);
            one_call(manager, reader, emu::FAIL_RUN, SIZE_MAX, {{1, 10, 0}, {2, 70, 0}, {3, 5, 0}}, 300);
            one_call(manager, reader, 0, 2, {{1, 10, 0}, {2, 70, 0}, {3, 5, 0}}, 0);
            one_call(manager, reader, 0, SIZE_MAX, {{1, 10, 0}, {100, 70, 0}, {3, 5, (uint64_t)TH_ERR_UNSUPPORTED}}, 300);
        }
    for (int k = 0; k < 20000; k++) {
        std::vector<emu::Request> reqs(r(0, 9));
        size_t need = 0;
        for (emu::Request &q : reqs) {
            q = emu::Request{r(0, 20) == 0 ? r(100, 200) : r(1, 100), r(0, 200), r(0, 25) == 0 ? (uint64_t)-(int64_t)r(1, 9) : 0};
            need = (need + 63) / 64 * 64 + q.length;
        }
        const size_t cap = r(0, 4) == 0 ? r(0, need + 1) : need + r(0, 70);  // (enough for either layout, or short of it)
        one_call((int)r(0, 2), (int)r(0, 2), r(0, 8) == 0 ? emu::FAIL_RUN : 0, r(0, 6) == 0 ? r(1, 9) : SIZE_MAX, reqs, cap);
    }
    std::printf("san_batched_reader: %zu calls, %zu refused, %zu short buffers, %zu failed runs: OK\n", calls, refused, short_buffers, failed_runs);
    return 0;
}
