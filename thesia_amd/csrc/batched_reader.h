// batched_reader.h — the one entry protocol of the batched readers (spectra, loudness meters, PCM export, figures, envelopes, waveform
// figures, formants) over either manager.  Plain C++17: no HIP header, no manager's definition, so that the protocol runs on the CPU
// (tests/emu/emu_batched_reader.cpp).
//
// A reader R is a traits struct (track_manager_internal.h has the seven):
//   Request, Info (derives from Public: what the check found, what the run needs), Public (the ABI's info), Out (the output's element)
//   unit               the word of the short-buffer message: "bytes", "floats", "doubles"
//   revision           which of the manager's revisions is stamped into every info
//   needs_colormap     the run reads the device colormap
//   run_updates_infos  the run writes into its infos: they are published again after it
//   out_optional       a NULL out is a size query that still runs (the meters' series); otherwise a NULL out is a short buffer
//   id_of(request)     the track, which decides the owner
//   check(owner, request, i, info*)   one request; i is its index in the batch, for the message
//   fit(info*, n)      a limit of the whole batch that a single owner reports before a short buffer (ReaderDefaults: none)
//   layout(info*, n)   every info's offset, in request order; returns the length of the whole output
//   run(owner, n, info*, out)         request i's result to out + info[i].offset and nowhere else
//
// A manager M is a small adaptor, made for one call:
//   null()                   the handle is NULL
//   before_lock(colormap)    what must happen before the shared lock is taken
//   lock()                   the manager's shared lock, held to the end of the call
//   revision(which)          the manager's own revision
//   single_owner             true: owner() is checked against and runs the caller's arrays as they are;
//                            false: n_slots(), find(id, &slot), owner(slot), lock_owner(slot), before_run(colormap, busy) and
//                            for_slots(busy, fn), which runs fn(slot) for the busy slots side by side and names a failing slot
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "common.h"

namespace th {
namespace br {

enum class Revision { waveform, spectrogram };

struct ReaderDefaults {
    static constexpr bool out_optional = false;
    template <class Info>
    static int fit(const Info *, size_t) { return TH_OK; }
};

// Layouts.  Records back to back, in elements of the output; `len` names the info's length member
template <class Info, class Len>
size_t layout_back_to_back(Info *info, size_t n, Len len) {
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        info[i].offset = info[i].plan.offset = at;
        at += info[i].*len;
    }
    return (size_t)at;
}
// Records of info.bytes at multiples of 64; returns the last record's end
template <class Info>
size_t layout_aligned_64(Info *info, size_t n) {
    uint64_t at = 0, end = 0;
    for (size_t i = 0; i < n; i++) {
        info[i].offset = info[i].plan.offset = at;
        end = at + info[i].bytes;
        at = (end + 63) & ~(uint64_t)63;
    }
    return (size_t)end;
}

// A batch of n requests split by owner (id_of(i): request i's track).  Every request is checked in request order against its owning
// slot, under that slot's shared lock (check(owner, i): the codes and the order of a single owner, the first faulty request decides).
// mine[s]: the requests of slot s in request order; busy: the slots that have any.  The caller holds the manager's lock.
struct Split {
    std::vector<std::vector<size_t>> mine;
    std::vector<uint32_t> busy;
};
template <class M, class IdOf, class Check>
int check_and_split(M &m, size_t n, IdOf id_of, Check check, Split *sp) {
    sp->mine.assign(m.n_slots(), {});
    for (size_t i = 0; i < n; i++) {
        uint32_t s = 0;
        if (!m.find(id_of(i), &s)) return fail(TH_ERR_NOT_FOUND, "Track %zu does not exist", (size_t)id_of(i));
        const auto sl = m.lock_owner(s);
        TH_CHECK(check(m.owner(s), i));
        sp->mine[s].push_back(i);
    }
    for (uint32_t s = 0; s < sp->mine.size(); s++)
        if (!sp->mine[s].empty()) sp->busy.push_back(s);
    return TH_OK;
}

// run(owner, idx) on every busy slot side by side, under the slot's shared lock; idx = mine[slot]
template <class M, class Run>
int run_on_owners(M &m, const Split &sp, Run run) {
    return m.for_slots(sp.busy, [&](uint32_t s) -> int {
        const auto sl = m.lock_owner(s);
        return run(m.owner(s), sp.mine[s]);
    });
}

// One slot's share of a run: its subset of the infos, in request order, with the offsets of the whole batch; what the run wrote into
// them goes back to their places (the slots' subsets are disjoint, so they may do this side by side)
template <class R, class Owner>
int run_subset(Owner *owner, const std::vector<size_t> &idx, typename R::Info *infos, typename R::Out *out) {
    std::vector<typename R::Info> sub(idx.size());
    for (size_t j = 0; j < idx.size(); j++) sub[j] = infos[idx[j]];
    TH_CHECK(R::run(owner, idx.size(), sub.data(), out));
    if constexpr (R::run_updates_infos)
        for (size_t j = 0; j < idx.size(); j++) infos[idx[j]] = sub[j];
    return TH_OK;
}

// The entry point of reader R on manager m.  In this order: NULL arguments; n == 0 is OK with *out_len = 0 and nothing else written;
// the first faulty request in request order decides; the infos (stamped with the manager's revision) and the length are published;
// a short buffer is reported; the run; the infos again where the run updates them (on a failed run the caller keeps what was
// published before it).  Nothing is written to out before the run.
template <class R, class M>
int batched_read(M m, const typename R::Request *reqs, size_t n, typename R::Out *out, size_t cap, typename R::Public *info,
                 size_t *out_len) {
    TH_REQUIRE(!m.null() && out_len && (n == 0 || (reqs && info)), "NULL argument");
    *out_len = 0;
    if (n == 0) return TH_OK;
    TH_CHECK(m.before_lock(R::needs_colormap));
    const auto rl = m.lock();
    std::vector<typename R::Info> infos(n);
    Split sp;
    if constexpr (M::single_owner) {
        for (size_t i = 0; i < n; i++) TH_CHECK(R::check(m.owner(), reqs[i], i, &infos[i]));
        TH_CHECK(R::fit(infos.data(), n));
    } else {
        TH_CHECK(check_and_split(m, n, [&](size_t i) { return R::id_of(reqs[i]); },
                                 [&](auto *owner, size_t i) { return R::check(owner, reqs[i], i, &infos[i]); }, &sp));
    }
    const size_t total = R::layout(infos.data(), n);
    const uint64_t revision = m.revision(R::revision);
    for (size_t i = 0; i < n; i++) {
        if constexpr (R::revision == Revision::waveform) infos[i].waveform_revision = revision;
        else infos[i].spectrogram_revision = revision;
        info[i] = infos[i];
    }
    *out_len = total;
    if (R::out_optional ? (out && cap < total) : (cap < total || !out))
        return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu %s", total, R::unit);
    if constexpr (M::single_owner) {
        TH_CHECK(R::run(m.owner(), n, infos.data(), out));
    } else {
        TH_CHECK(m.before_run(R::needs_colormap, sp.busy));
        TH_CHECK(run_on_owners(m, sp, [&](auto *owner, const std::vector<size_t> &idx) { return run_subset<R>(owner, idx, infos.data(), out); }));
    }
    if constexpr (R::run_updates_infos)
        for (size_t i = 0; i < n; i++) info[i] = infos[i];
    return TH_OK;
}

// The single-request form of a batched entry: batch(&one, &len) is the batch call for the one request; the caller's info is
// written when the batch call published one (OK or a short buffer)
template <class Public, class Batch>
int single_read(Public *info, Batch batch) {
    Public one{};
    size_t len = 0;
    const int rc = batch(&one, &len);
    if (info && (rc == TH_OK || rc == TH_ERR_BUFFER_TOO_SMALL)) *info = one;
    return rc;
}

}  // namespace br
}  // namespace th
