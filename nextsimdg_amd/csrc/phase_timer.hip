// phase_timer.hip -- per-phase device timing of a model step: marks on the context's stream (include/nsdg.h "per-phase device timing").
//
// Every mark records ONE event; the interval between two consecutive marks belongs to the phase the first one opened, so the phases
// of a span share their boundary timestamps and their times add up to the span's own hipEventElapsedTime(first, end) but for the
// float roundings of that call.  The events come from a fixed pool of NSDG_PHASE_RING; the marks that have not been read yet wait in a
// FIFO of the same length.  A mark is read -- its interval and, for an NSDG_PHASE_END, its span added to the table -- as soon as its event
// has completed: at the next nsdg_phase_mark (hipEventQuery, front of the FIFO first, stopping at the first event that is not ready)
// or at nsdg_phase_times.  Reading a mark returns the PREVIOUS mark's event to the pool, except the one that opened the running span,
// which is kept until the span's end has been read.  So the pool runs dry only when NSDG_PHASE_RING - 1 marks are outstanding, and then
// the mark waits for the oldest of them; nothing is ever recycled unread (unlike the exchange timing's ring, halo.hip, which
// reports such pairs as `untimed`: a step's phase table has to add up).
#include <chrono>

#include "nsdg_internal.h"

struct nsdg_phase_timer {
    static constexpr int RING = NSDG_PHASE_RING;
    bool enabled = false;
    hipEvent_t pool[RING] = {}; // free events, [0, nfree)
    int nfree = 0;
    struct Mark {
        hipEvent_t ev;
        int phase;
    };
    Mark fifo[RING]; // recorded, not yet read: [head, head + pending) modulo RING
    int head = 0, pending = 0;
    int issued_open = -1; // the phase the last RECORDED mark opened (-1: none runs)
    // state of the last READ mark
    hipEvent_t prev = nullptr; // its event, while the phase it opened is not closed
    int open = -1; // that phase
    hipEvent_t span_first = nullptr; // the mark that opened the running span
    nsdg_phase_table table = {};
};

namespace {

void release(nsdg_phase_timer* t, hipEvent_t ev) { t->pool[t->nfree++] = ev; }

// adds the front mark of the FIFO, whose event has completed, to the table
int read_front(nsdg_phase_timer* t)
{
    const nsdg_phase_timer::Mark m = t->fifo[t->head];
    if (t->open >= 0) {
        float ms = 0.f;
        NSDG_CHECK_HIP(hipEventElapsedTime(&ms, t->prev, m.ev));
        t->table.ms[t->open] += (double)ms;
        ++t->table.count[t->open];
    }
    if (m.phase == NSDG_PHASE_END && t->span_first) {
        float ms = 0.f;
        NSDG_CHECK_HIP(hipEventElapsedTime(&ms, t->span_first, m.ev));
        t->table.total_ms += (double)ms;
        ++t->table.spans;
        if (t->span_first != t->prev)
            release(t, t->span_first);
        t->span_first = nullptr;
    }
    if (t->prev && t->prev != t->span_first)
        release(t, t->prev);
    t->head = (t->head + 1) % nsdg_phase_timer::RING;
    --t->pending;
    if (m.phase == NSDG_PHASE_END) {
        release(t, m.ev);
        t->prev = nullptr;
        t->open = -1;
    } else {
        t->prev = m.ev;
        t->open = m.phase;
        if (!t->span_first)
            t->span_first = m.ev;
    }
    return NSDG_OK;
}

// reads every mark whose event has completed, in order; never waits
int harvest(nsdg_phase_timer* t)
{
    while (t->pending > 0) {
        const hipError_t e = hipEventQuery(t->fifo[t->head].ev);
        if (e == hipErrorNotReady) {
            (void)hipGetLastError();
            return NSDG_OK;
        }
        NSDG_CHECK_HIP(e);
        const int rc = read_front(t);
        if (rc != NSDG_OK)
            return rc;
    }
    return NSDG_OK;
}

// the pool is dry: wait for the oldest outstanding mark (on a context with a communicator not beyond its deadline) and read it
int wait_oldest(nsdg_ctx* ctx, nsdg_phase_timer* t)
{
    hipEvent_t ev = t->fifo[t->head].ev;
    if (ctx->comm && ctx->comm_deadline_s > 0.) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t e = hipEventQuery(ev);
            if (e == hipSuccess)
                break;
            if (e != hipErrorNotReady) {
                nsdg_set_error("nsdg_phase_mark: hipEventQuery failed: %s", hipGetErrorString(e));
                return NSDG_ERR_HIP;
            }
            (void)hipGetLastError();
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > ctx->comm_deadline_s) {
                nsdg_set_error("nsdg_phase_mark: the oldest of %d outstanding marks did not complete within %g s", t->pending, ctx->comm_deadline_s);
                return NSDG_ERR_COMM;
            }
        }
    } else {
        NSDG_CHECK_HIP(hipEventSynchronize(ev));
    }
    return read_front(t);
}

void forget(nsdg_phase_timer* t)
{
    // back to the state of a fresh timer; events that are still outstanding may be recorded again (hipEventRecord replaces the earlier record)
    while (t->pending > 0) {
        release(t, t->fifo[t->head].ev);
        t->head = (t->head + 1) % nsdg_phase_timer::RING;
        --t->pending;
    }
    if (t->span_first && t->span_first != t->prev)
        release(t, t->span_first);
    if (t->prev)
        release(t, t->prev);
    t->prev = t->span_first = nullptr;
    t->open = t->issued_open = -1;
    t->head = 0;
    t->table = nsdg_phase_table {};
}

} // namespace

void nsdg_phase_timer_free(nsdg_ctx* ctx)
{
    nsdg_phase_timer* t = ctx->phase;
    if (!t)
        return;
    forget(t);
    for (int k = 0; k < t->nfree; ++k)
        (void)hipEventDestroy(t->pool[k]);
    delete t;
    ctx->phase = nullptr;
}

extern "C" {

int nsdg_phase_timing_set(nsdg_ctx* ctx, int32_t enable)
{
    NSDG_CHECK_ARG(ctx != nullptr, "null context");
    nsdg_phase_timer* t = ctx->phase;
    if (!enable) {
        if (t) {
            forget(t);
            t->enabled = false;
        }
        return NSDG_OK;
    }
    if (!t) {
        NSDG_CHECK_HIP(hipSetDevice(ctx->device));
        t = new nsdg_phase_timer();
        ctx->phase = t; // from here on nsdg_ctx_destroy frees what exists
        for (int k = 0; k < nsdg_phase_timer::RING; ++k) {
            hipEvent_t ev = nullptr;
            NSDG_CHECK_HIP(hipEventCreate(&ev));
            release(t, ev);
        }
    }
    t->enabled = true;
    return NSDG_OK;
}

int nsdg_phase_mark(nsdg_ctx* ctx, int32_t phase)
{
    NSDG_CHECK_ARG(ctx != nullptr, "null context");
    NSDG_CHECK_ARG(phase == NSDG_PHASE_END || (phase >= 0 && phase < NSDG_PHASE_MAX), "phase must be in [0, NSDG_PHASE_MAX) or NSDG_PHASE_END");
    nsdg_phase_timer* t = ctx->phase;
    if (!t || !t->enabled)
        return NSDG_OK;
    if (phase == NSDG_PHASE_END && t->issued_open < 0)
        return NSDG_OK; // nothing runs: nothing to close
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    NSDG_CHECK_HIP(hipStreamIsCapturing(ctx->stream, &cap));
    if (cap != hipStreamCaptureStatusNone) {
        nsdg_set_error("nsdg_phase_mark: the context's stream is being captured; mark between the captured regions");
        return NSDG_ERR_STATE;
    }
    int rc = harvest(t);
    while (rc == NSDG_OK && t->nfree == 0)
        rc = wait_oldest(ctx, t);
    if (rc != NSDG_OK)
        return rc;
    hipEvent_t ev = t->pool[t->nfree - 1];
    NSDG_CHECK_HIP(hipEventRecord(ev, ctx->stream));
    --t->nfree;
    t->fifo[(t->head + t->pending) % nsdg_phase_timer::RING] = nsdg_phase_timer::Mark { ev, (int)phase };
    ++t->pending;
    t->issued_open = phase == NSDG_PHASE_END ? -1 : (int)phase;
    return NSDG_OK;
}

int nsdg_phase_times(nsdg_ctx* ctx, nsdg_phase_table* out, int32_t reset)
{
    NSDG_CHECK_ARG(ctx != nullptr, "null context");
    NSDG_CHECK_ARG(out != nullptr, "null output pointer");
    *out = nsdg_phase_table {};
    nsdg_phase_timer* t = ctx->phase;
    if (!t || !t->enabled)
        return NSDG_OK;
    if (t->pending > 0) {
        if (ctx->comm) { // a dead neighbour must not block this rank for ever
            const int rc = nsdg_comm_bounded_drain(ctx);
            if (rc != NSDG_OK)
                return rc;
        } else {
            NSDG_CHECK_HIP(hipEventSynchronize(t->fifo[(t->head + t->pending - 1) % nsdg_phase_timer::RING].ev));
        }
        while (t->pending > 0) {
            const int rc = read_front(t);
            if (rc != NSDG_OK)
                return rc;
        }
    }
    *out = t->table;
    if (reset)
        t->table = nsdg_phase_table {};
    return NSDG_OK;
}

} // extern "C"
