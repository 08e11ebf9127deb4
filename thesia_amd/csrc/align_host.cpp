// align_host.cpp — the host entries of the alignment reader (include/thesia_amd.h "Align two tracks"): th_align_plan_for, th_xcorr_f64,
// th_align_energy_f64, th_align_peak and th_align_f64 over align_plan.h, with the statuses and messages of the C ABI.  No HIP.
#include <cstdint>

#include "align_plan.h"
#include "common.h"

using namespace th;

namespace {
int plan_checked(uint32_t sr_ref, size_t n_ref, uint32_t sr, size_t n, const th_align_request *req, th_align_plan *pl) {
    const int rc = align_plan_for(sr_ref, n_ref, sr, n, *req, pl);
    TH_REQUIRE(rc != 1,
               "bad alignment request: [%g, %g) s of %zu samples at %u Hz against %zu samples at %u Hz, lags up to %g s, which %u / %u, kind "
               "%u, flags %u",
               req->start_sec, req->end_sec, n_ref, sr_ref, n, sr, req->max_lag_sec, req->ref_which, req->which, req->kind, req->flags);
    if (rc != 0)
        return fail(TH_ERR_UNSUPPORTED,
                    "alignment of [%g, %g) s at %u Hz against %u Hz over %g s of lag: the rates must be equal, the range at most %u samples, "
                    "the lag at most %u samples, their product at most 2^40",
                    req->start_sec, req->end_sec, sr_ref, sr, req->max_lag_sec, TH_ALIGN_MAX_REF, TH_ALIGN_MAX_LAG);
    return TH_OK;
}
}  // namespace

TH_API int th_align_plan_for(uint32_t sr_ref, size_t n_ref, uint32_t sr, size_t n, const th_align_request *req, th_align_plan *plan) {
    TH_TRY
    TH_REQUIRE(req && plan, "NULL argument");
    return plan_checked(sr_ref, n_ref, sr, n, req, plan);
    TH_CATCH
}

TH_API int th_xcorr_f64(const float *a, size_t n_a, const float *b, size_t n_b, int64_t first, size_t n_lags, double *r) {
    TH_TRY
    TH_REQUIRE((n_a == 0 || a) && (n_b == 0 || b) && (n_lags == 0 || r), "NULL argument");
    TH_REQUIRE(n_a <= TH_ALIGN_MAX_REF && n_lags <= 2 * (size_t)TH_ALIGN_MAX_LAG + 1, "%zu reference samples (at most %u), %zu lags (at most %zu)",
               n_a, TH_ALIGN_MAX_REF, n_lags, 2 * (size_t)TH_ALIGN_MAX_LAG + 1);
    TH_REQUIRE(first >= -((int64_t)1 << 62) && first <= ((int64_t)1 << 62), "first index %lld", (long long)first);
    xcorr_f64(a, n_a, b, n_b, first, n_lags, r);
    return TH_OK;
    TH_CATCH
}

TH_API int th_align_energy_f64(const float *x, size_t n, int64_t first, size_t n_sum, double *energy) {
    TH_TRY
    TH_REQUIRE((n == 0 || x) && energy, "NULL argument");
    TH_REQUIRE(n_sum <= TH_ALIGN_MAX_REF, "%zu samples (at most %u)", n_sum, TH_ALIGN_MAX_REF);
    TH_REQUIRE(first >= -((int64_t)1 << 62) && first <= ((int64_t)1 << 62), "first index %lld", (long long)first);
    *energy = align_energy_f64(x, n, first, n_sum);
    return TH_OK;
    TH_CATCH
}

TH_API int th_align_peak(const double *r, size_t n_lags, uint32_t flags, double e_ref, uint32_t *status, size_t *peak, double *delta,
                         double *polarity) {
    TH_TRY
    TH_REQUIRE((n_lags == 0 || r) && status && peak && delta && polarity, "NULL argument");
    TH_REQUIRE(!(flags & ~TH_ALIGN_ABS), "unknown flags %u", flags);
    const AlignPeak pk = align_peak(r, n_lags, flags, e_ref);
    *status = pk.status;
    *peak = (size_t)pk.index;
    *delta = pk.delta;
    *polarity = pk.polarity;
    return TH_OK;
    TH_CATCH
}

TH_API int th_align_f64(const float *ref, size_t n_ref, uint32_t sr_ref, const float *probe, size_t n, uint32_t sr,
                        const th_align_request *req, double *out, size_t cap_doubles, size_t *out_len) {
    TH_TRY
    TH_REQUIRE(req && out_len && (n_ref == 0 || ref) && (n == 0 || probe), "NULL argument");
    *out_len = 0;
    th_align_plan pl;
    TH_CHECK(plan_checked(sr_ref, n_ref, sr, n, req, &pl));
    *out_len = (size_t)pl.length;
    if (!out || cap_doubles < pl.length) return fail(TH_ERR_BUFFER_TOO_SMALL, "need %zu doubles", (size_t)pl.length);
    align_f64(ref, probe, n, pl, out);
    return TH_OK;
    TH_CATCH
}
