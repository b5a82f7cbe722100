// Driver of tests/test_draw_sched.py: one whole ahmc_sample call's sampling phase through the launch-length controller
// (csrc/ahmc_draw_sched.hpp), the way sample_run / sample_draws_launch (csrc/ahmc_sample_host.hpp) drive it — with a table in the
// place of the clock.  Built by the test itself with the host compiler: the controller includes nothing of HIP.
#include "ahmc_draw_sched.hpp"

// state: phase, len, best_len, primed, g_len, g_left (in / out, with *best_thr); thr_by_len[L] = throughput of a timed group of
// launches of L transitions, L < n_thr.  out: (k, probing, phase after, best_len after) per launch; the call is cut off after `cap`
// launches (a call that failed half way).  Returns the number of launches, or -1 (a launch length outside the table).
extern "C" int64_t draw_sched_run(int64_t left, int64_t batch, int64_t draw_batch, int32_t sched, int32_t order_refresh_env, int32_t first_batch,
                                  int32_t* order_from_work, int32_t eps_scalar, int64_t* state, double* best_thr, const double* thr_by_len,
                                  int64_t n_thr, int64_t* out, int64_t cap) {
  ahmc::DrawSched sc;
  sc.phase = (int)state[0]; sc.len = state[1]; sc.best_len = state[2]; sc.primed = state[3] != 0; sc.g_len = state[4]; sc.g_left = (int)state[5];
  sc.best_thr = *best_thr;
  const bool order_refresh = order_refresh_env != 0 && eps_scalar == 0;   // (no dense engine here)
  int64_t n = 0;
  sc.drop_group();   // the call's entry
  while (left > 0 && n < cap) {
    const ahmc::DrawSched::Plan pl = sc.plan(left, batch, draw_batch, sched != 0 && order_refresh, first_batch, *order_from_work != 0, eps_scalar != 0);
    if (pl.k < 1 || pl.k >= n_thr) return -1;
    if (order_refresh && pl.k >= 2) *order_from_work = 1;   // the launch's work re-sorted the dispatch order
    if (pl.probing) sc.timed_launch_done();
    if (pl.ends) sc.close_group(pl.k, thr_by_len[pl.k], batch);
    out[4 * n + 0] = pl.k; out[4 * n + 1] = pl.probing; out[4 * n + 2] = sc.phase; out[4 * n + 3] = sc.best_len;
    ++n;
    left -= pl.k;
  }
  state[0] = sc.phase; state[1] = sc.len; state[2] = sc.best_len; state[3] = sc.primed; state[4] = sc.g_len; state[5] = sc.g_left;
  *best_thr = sc.best_thr;
  return n;
}
