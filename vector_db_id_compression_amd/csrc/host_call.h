// host_call.h -- the host frame of a C-ABI entry point, shared by the four codec translation units: the ev0 .. ev1 kernel timer, the
// wait-on-early-return guard, the lazy host mirror of an object's offsets and the request preambles of decode_lists / get.  Host code
// only; nothing here launches a kernel of its own.
#pragma once
#include "common.h"

// Kernel time of a call: ctx->ev0 .. ctx->ev1 on the context's stream.  The timer holds no state but the context, so a start recorded
// by a helper is read by a timer of its caller, work may be enqueued between mark() and the call's wait, and a second interval
// (ev_chain, ev_pre) is added by the call that owns it.  No event or allocation of its own; the only host waits are stop()'s (for ev1)
// and finish()'s (the call's own wait for the stream).
struct EventTimer {
    vidc_ctx *c;
    explicit EventTimer(vidc_ctx *ctx) : c(ctx) {}
    // (ROC's form: started where it is declared, the records unchecked)
    static EventTimer started(vidc_ctx *ctx) {
        EventTimer t(ctx);
        (void)t.start();
        return t;
    }
    hipError_t start() { return hipEventRecord(c->ev0, c->stream); }
    hipError_t mark() { return hipEventRecord(c->ev1, c->stream); }
    // after the caller's wait for the stream (or for ev1)
    double elapsed() const {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        return ms;
    }
    // mark + a wait for ev1 alone + elapsed
    double stop() {
        (void)mark();
        (void)vidc::vidc_event_wait(c->ev1);
        return elapsed();
    }
    // the tail of a call that enqueues nothing behind its last kernel: mark, the call's one wait, last_kernel_ms.  A VIDC_* status
    // (VIDC_TRY at the call site): the error text names the HIP call that failed
    int finish() {
        VIDC_HIP(hipEventRecord(c->ev1, c->stream));
        VIDC_HIP(vidc::vidc_stream_wait(c->stream));
        c->last_kernel_ms = elapsed();
        return VIDC_OK;
    }
};

// Waits for the context's stream when the scope is left while armed: an early return must not hand staging blocks back to the pool
// while copies or kernels in flight still use them.  Declare it BEHIND the blocks it protects (destroyed first); disarm() once the
// call has waited itself.
struct StreamGuard {
    vidc_ctx *c;
    bool armed;
    explicit StreamGuard(vidc_ctx *ctx, bool armed_ = true) : c(ctx), armed(armed_) {}
    StreamGuard(const StreamGuard &) = delete;
    StreamGuard &operator=(const StreamGuard &) = delete;
    ~StreamGuard() { if (armed) (void)vidc::vidc_stream_wait(c->stream); }
    void arm() { armed = true; }
    void disarm() { armed = false; }
};

// lazy host mirrors of device-resident metadata (blocking copies; everything was synchronised when the object was built).  The
// object's own vector is resized in place: no trip through vec_pool on this path (the objects' destructors may still give it back)
template <typename T>
inline int mirror_to_host(std::vector<T> &dst, const T *d_src, size_t count) {
    dst.resize(count);
    if (count) VIDC_HIP(hipMemcpy(dst.data(), d_src, count * sizeof(T), hipMemcpyDeviceToHost));
    return VIDC_OK;
}
// the host mirror of the offsets of an object built from device offsets, on first use (one copy of nlist + 1 words).  Obj: mu,
// offsets, offsets_host, device, nlist.  _locked: the caller holds o->mu.
template <typename Obj>
inline int ensure_offsets_host_locked(const Obj *o, const uint64_t *d_offsets) {
    if (o->offsets_host) return VIDC_OK;
    VIDC_HIP(hipSetDevice(o->device));
    VIDC_TRY(mirror_to_host(o->offsets, d_offsets, o->nlist + 1));
    o->offsets_host = true;
    return VIDC_OK;
}
template <typename Obj>
inline int ensure_offsets_host(const Obj *o, const uint64_t *d_offsets) {
    std::lock_guard<std::mutex> g(o->mu);
    return ensure_offsets_host_locked(o, d_offsets);
}

// vidc_*_decode_lists: the range check of the request and out_offsets[m + 1], the prefix sum of the requested lists' sizes
inline int lists_request_offsets(uint64_t nlist, const std::vector<uint64_t> &offsets, uint64_t m, const uint64_t *list_nos,
                                 uint64_t *out_offsets) {
    out_offsets[0] = 0;
    for (uint64_t i = 0; i < m; i++) {
        if (list_nos[i] >= nlist) { vidc::set_error("list number out of range"); return VIDC_ERR_INVALID; }
        out_offsets[i + 1] = out_offsets[i] + (offsets[list_nos[i] + 1] - offsets[list_nos[i]]);
    }
    return VIDC_OK;
}

// vidc_*_get / vidc_wt_select (m > 0, arrays checked by the caller): every (list, offset) checked against the host offsets before any
// device work, the request staged in the context's block cache, launch(d_list_nos, d_offs, d_ids), 8 * m bytes copied back, one wait.
template <typename Launch>
inline int get_request(vidc_ctx *ctx, const char *what, uint64_t nlist, const std::vector<uint64_t> &offsets, uint64_t m,
                       const uint64_t *list_nos, const uint64_t *offs, int64_t *ids_out, Launch &&launch) {
    for (uint64_t i = 0; i < m; i++)
        if (list_nos[i] >= nlist || offs[i] >= offsets[list_nos[i] + 1] - offsets[list_nos[i]]) {
            vidc::set_error("%s: (list %llu, offset %llu) out of range", what, (unsigned long long)list_nos[i], (unsigned long long)offs[i]);
            return VIDC_ERR_INVALID;
        }
    VIDC_HIP(hipSetDevice(ctx->device));
    vidc::Scratch s_l, s_o, s_r;
    VIDC_TRY(s_l.get(ctx, m * 8)); VIDC_TRY(s_o.get(ctx, m * 8)); VIDC_TRY(s_r.get(ctx, m * 8));
    VIDC_HIP(hipMemcpyAsync(s_l.p, list_nos, m * 8, hipMemcpyHostToDevice, ctx->stream));
    VIDC_HIP(hipMemcpyAsync(s_o.p, offs, m * 8, hipMemcpyHostToDevice, ctx->stream));
    launch(s_l.as<uint64_t>(), s_o.as<uint64_t>(), s_r.as<int64_t>());
    VIDC_HIP(hipGetLastError());
    VIDC_HIP(hipMemcpyAsync(ids_out, s_r.p, m * 8, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    ctx->d2h_bytes += m * 8;
    return VIDC_OK;
}
