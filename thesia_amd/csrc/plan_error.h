// plan_error.h — how a host planner (stft_plan.h, reader_plan.h, batch_plan.h style: plain data, no HIP) refuses: a default-made plan
// with err and err_text set.
#pragma once
#include <cstdarg>
#include <cstdio>

namespace th {
template <class P>
P plan_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
template <class P>
P plan_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    P p;
    p.err = code;
    p.err_text = buf;
    return p;
}
}  // namespace th
