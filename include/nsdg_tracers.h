/* nsdg_tracers.h -- the "ice tracers" section of the C ABI of libnsdg.so (csrc/tracers.hip).  include/nsdg.h
 * includes this file: a caller of the library includes nsdg.h and has these calls with it.  The section is a header of its own with
 * tables of its own: abi.TRACER_SYMBOLS binds its functions, tests/test_gpu_tracers_stream_order.py holds each of them to stream order.
 * Plain C99, like nsdg.h. */
#ifndef NSDG_TRACERS_H
#define NSDG_TRACERS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct nsdg_ctx;

/* ---- ice tracers: ice age and passive tracers ride on the moving ice ------------------------------------------------------------------
 * The scheme of the column state transport for up to NSDG_TRACERS_MAX intensive quantities T_k (one plane each, DG0) at once: each travels
 * as the conserved product Q_k = H T_k with the ice volume, rebuilt before every transport step and divided back after it.  The Q_k are
 * advected in a transport run of their own (unbounded: no limiter, no cap), after the run of H, A and the other fields and with the same
 * prepared velocity; sum_e mean(H)_e T_k,e is conserved by it up to rounding.  T, Q and kind are host arrays of n device pointers / ints.
 * Every operation below is one IEEE fp64 operation.
 *
 * nsdg_tracers_weight: Q[k][c*nx*ny + e] = T[k][e] * H[c*nx*ny + e] for c < nc(order), k < n and the elements e of rows [j0, j1): bit for
 * bit what n calls of nsdg_tracer_weight give, in one launch that loads the planes of H once.
 * nsdg_tracers_recover: the ice test of nsdg_tracer_recover on the means of H and A (false for a NaN).  Where it holds, t = Q[k][e] / H[e]
 * and T[k][e] = t + dt for kind[k] == NSDG_TRACER_AGE, t for NSDG_TRACER_PASSIVE; where it does not, T[k][e] = 0 for both kinds: a
 * tracer is zero where there is no ice.
 * nsdg_tracers_dilute: the thermodynamic source -- ice that grows carries the value 0, ice that melts has the mean value.  h_before and
 * h_after are planes [ny][nx] of the mean thickness around the column step.  With hb = h_before[e] > 0 ? h_before[e] : 0 (a NaN counts as
 * 0) and ha = h_after[e]: !(ha > 0): T[k][e] = 0; else ha > hb: T[k][e] = (T[k][e] * hb) / ha; otherwise T[k][e] is unchanged.
 *
 * All three are element-local (a row block runs them on its ghost rows too), stream-ordered and one launch each.  Checks, as for
 * nsdg_tracer_*: grid set (else NSDG_ERR_STATE); an order outside 0..2, a row range outside the local array, a null pointer (the arrays or
 * one of their n entries), n outside 1..NSDG_TRACERS_MAX, an unknown kind; a Q[k] that overlaps H, any T[j] or another Q[j] (weight); a
 * T[k] that overlaps H, A, any Q[j] or another T[j] (recover), h_before, h_after or another T[j] (dilute) -- nc(order) nx ny doubles of a DG
 * field, nx ny of a plane: NSDG_ERR_ARG, and nothing is launched.  j0 == j1 does nothing. */
#define NSDG_TRACERS_MAX 4
enum { NSDG_TRACER_PASSIVE = 0, NSDG_TRACER_AGE = 1 };
int nsdg_tracers_weight(struct nsdg_ctx* ctx, int32_t order, int32_t j0, int32_t j1, const double* H, int32_t n, const double* const* T,
    double* const* Q);
int nsdg_tracers_recover(struct nsdg_ctx* ctx, int32_t order, int32_t j0, int32_t j1, const double* H, const double* A, int32_t n,
    const double* const* Q, const int32_t* kind, double dt, double min_conc, double min_thick, double* const* T);
int nsdg_tracers_dilute(struct nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* h_before, const double* h_after, int32_t n, double* const* T);

#ifdef __cplusplus
}
#endif

#endif /* NSDG_TRACERS_H */
