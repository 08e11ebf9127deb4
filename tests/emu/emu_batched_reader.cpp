// emu_batched_reader.cpp — br::batched_read (thesia_amd/csrc/batched_reader.h) over fake readers and fake managers, on the CPU.
// The fakes record what the driver asks of them, in order, so that tests/test_batched_reader_host.py can assert the entry protocol
// clause by clause; scripts/san_batched_reader.cpp includes this file and runs the same calls under the sanitizers.
//
// Managers: 0 = one owner (tracks 1 .. 99), 1 = two owners (odd ids on slot 0, even ids on slot 1, up to 99), 2 = a NULL handle.
// Readers (all write bytes): 0 = records at multiples of 64, spectrogram revision, needs the colormap, its run leaves the infos alone;
// 1 = records back to back, waveform revision, its run counts into the infos; 2 = as 1 with an optional output.
// A request is (id, length, fault): a fault != 0 makes its check fail with that code.  A run writes byte (id & 255) over its record.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../thesia_amd/csrc/batched_reader.h"

namespace th {
static thread_local char last_error[512];
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
}
const char *get_error() { return last_error; }
}  // namespace th

namespace emu {
using namespace th;

enum Event : uint64_t { BEFORE_LOCK = 1, LOCK, LOCK_OWNER, CHECK, FIT, REVISION, BEFORE_RUN, RUN };
enum Flag : int { REQS_NULL = 1, INFO_NULL = 2, OUT_NULL = 4, LEN_NULL = 8, FAIL_RUN = 16 };  // FAIL_RUN: the last owner's run fails

struct Held {  // a fake lock
    ~Held() {}
};
struct Owner {
    uint32_t slot;
    bool fail_run;
    std::vector<uint64_t> *log;
};

struct Request {
    uint64_t id, length, fault;
};
struct PublicInfo {
    uint64_t offset, length, bytes, waveform_revision, spectrogram_revision, count;
};
struct Info : PublicInfo {
    struct {
        uint64_t offset;
    } plan;
    uint64_t id;
};

size_t fit_limit = SIZE_MAX;  // a batch of more requests does not fit

template <bool Aligned, bool Updates, bool Optional>
struct Reader : br::ReaderDefaults {
    using Request = emu::Request;
    using Info = emu::Info;
    using Public = PublicInfo;
    using Out = uint8_t;
    static constexpr const char *unit = Aligned ? "bytes" : "doubles";
    static constexpr br::Revision revision = Aligned ? br::Revision::spectrogram : br::Revision::waveform;
    static constexpr bool needs_colormap = Aligned, run_updates_infos = Updates, out_optional = Optional;
    static size_t id_of(const Request &r) { return (size_t)r.id; }
    static int check(Owner *o, const Request &r, size_t i, Info *info) {
        o->log->insert(o->log->end(), {CHECK, o->slot, i});
        if (r.id >= 100) return fail(TH_ERR_NOT_FOUND, "request %zu: Track %zu does not exist", i, (size_t)r.id);
        if (r.fault) return fail((int)r.fault, "request %zu: fault %d", i, (int)r.fault);
        *info = Info{};
        info->length = info->bytes = r.length;
        info->waveform_revision = info->spectrogram_revision = 7777;  // (an owner's own: the driver's stamp replaces it)
        info->id = r.id;
        return TH_OK;
    }
    static int fit(const Info *, size_t n) {
        if (n > fit_limit) return fail(TH_ERR_INVALID_ARG, "at most %zu requests per call", fit_limit);
        return TH_OK;
    }
    static size_t layout(Info *info, size_t n) {
        if constexpr (Aligned) return br::layout_aligned_64(info, n);
        else return br::layout_back_to_back(info, n, &Info::length);
    }
    static int run(Owner *o, size_t n, Info *info, Out *out) {
        o->log->insert(o->log->end(), {RUN, o->slot, n});
        for (size_t i = 0; i < n; i++) {
            o->log->insert(o->log->end(), {info[i].id, info[i].offset, info[i].plan.offset, info[i].waveform_revision, info[i].spectrogram_revision});
            info[i].count = 1000 + info[i].id;
            if (out) std::memset(out + info[i].offset, (int)(info[i].id & 255), (size_t)info[i].length);
        }
        if (o->fail_run) return fail(TH_ERR_HIP, "the run failed");
        return TH_OK;
    }
};

struct Manager {
    std::vector<uint64_t> *log;
    Owner *owners;
    bool is_null;
    bool null() const { return is_null; }
    int before_lock(bool colormap) const {
        log->insert(log->end(), {BEFORE_LOCK, colormap});
        return TH_OK;
    }
    Held lock() const {
        log->push_back(LOCK);
        return {};
    }
    uint64_t revision(br::Revision which) const {
        log->insert(log->end(), {REVISION, which == br::Revision::waveform ? 0u : 1u});
        return which == br::Revision::waveform ? 41 : 42;
    }
};
struct Single : Manager {
    static constexpr bool single_owner = true;
    Owner *owner() const { return &owners[0]; }
};
struct Multi : Manager {
    static constexpr bool single_owner = false;
    size_t n_slots() const { return 2; }
    bool find(size_t id, uint32_t *slot) const {
        *slot = id % 2 ? 0 : 1;
        return id < 100;
    }
    Owner *owner(uint32_t s) const { return &owners[s]; }
    Held lock_owner(uint32_t s) const {
        log->insert(log->end(), {LOCK_OWNER, s});
        return {};
    }
    int before_run(bool colormap, const std::vector<uint32_t> &busy) const {
        log->insert(log->end(), {BEFORE_RUN, colormap, busy.size()});
        log->insert(log->end(), busy.begin(), busy.end());
        return TH_OK;
    }
    template <class F>
    int for_slots(const std::vector<uint32_t> &which, F fn) const {  // one after the other; every slot runs, the first failure is reported
        int rc = TH_OK;
        uint32_t failed = 0;
        std::string msg;
        for (uint32_t s : which) {
            const int r = fn(s);
            if (r != TH_OK && rc == TH_OK) {
                rc = r;
                failed = s;
                msg = get_error();
            }
        }
        return rc == TH_OK ? TH_OK : fail(rc, "slot %u (device %d): %s", failed, 0, msg.c_str());
    }
};

template <class R>
int call(int manager, int flags, const Request *reqs, size_t n, uint8_t *out, size_t cap, PublicInfo *info, size_t *out_len,
         std::vector<uint64_t> *log) {
    Owner owners[2] = {{0, manager == 0 && (flags & FAIL_RUN), log}, {1, manager == 1 && (flags & FAIL_RUN), log}};
    if (flags & REQS_NULL) reqs = nullptr;
    if (flags & INFO_NULL) info = nullptr;
    if (flags & OUT_NULL) out = nullptr;
    if (flags & LEN_NULL) out_len = nullptr;
    if (manager == 1) return br::batched_read<R>(Multi{{log, owners, false}}, reqs, n, out, cap, info, out_len);
    return br::batched_read<R>(Single{{log, owners, manager == 2}}, reqs, n, out, cap, info, out_len);
}

}  // namespace emu

// reqs: n x (id, length, fault); info: n x 6 (PublicInfo); log: the events, *log_len of them (at most log_cap are written)
extern "C" __attribute__((visibility("default"))) int emu_batched_reader(int manager, int reader, int flags, uint64_t fit_limit,
                                                                         const uint64_t *reqs, size_t n, uint8_t *out, size_t cap,
                                                                         uint64_t *info, uint64_t *out_len, char *msg, size_t msg_cap,
                                                                         uint64_t *log, size_t log_cap, size_t *log_len) {
    static_assert(sizeof(emu::Request) == 3 * sizeof(uint64_t) && sizeof(emu::PublicInfo) == 6 * sizeof(uint64_t), "packed as the caller's rows");
    std::vector<uint64_t> events;
    emu::fit_limit = (size_t)fit_limit;
    const emu::Request *rq = reinterpret_cast<const emu::Request *>(reqs);
    emu::PublicInfo *pi = reinterpret_cast<emu::PublicInfo *>(info);
    size_t len = out_len ? (size_t)*out_len : 0;
    th::set_error("%s", "");
    int rc;
    if (reader == 0) rc = emu::call<emu::Reader<true, false, false>>(manager, flags, rq, n, out, cap, pi, &len, &events);
    else if (reader == 1) rc = emu::call<emu::Reader<false, true, false>>(manager, flags, rq, n, out, cap, pi, &len, &events);
    else rc = emu::call<emu::Reader<false, true, true>>(manager, flags, rq, n, out, cap, pi, &len, &events);
    if (out_len) *out_len = len;
    if (msg && msg_cap) std::snprintf(msg, msg_cap, "%s", th::get_error());
    *log_len = events.size();
    for (size_t i = 0; i < events.size() && i < log_cap; i++) log[i] = events[i];
    return rc;
}

// br::single_read: the caller's info is written exactly when the batch call published one
extern "C" __attribute__((visibility("default"))) int emu_single_read(int rc_of_batch, uint64_t *info) {
    return th::br::single_read(info, [&](uint64_t *one, size_t *len) {
        *one = 5 + *len;
        return rc_of_batch;
    });
}
