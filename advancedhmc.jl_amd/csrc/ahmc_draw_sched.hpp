// ahmc_draw_sched.hpp — the launch-length controller of the sampling phase (round 4), as plain C++: no HIP, no clock.
// The sampling loop (ahmc_sample_host.hpp: sample_draws_launch) asks it for the length of the next launch, does the device work
// of a timed group's two ends itself, measures the group's throughput and hands it in.  tests/test_draw_sched.py replays whole
// calls through tests/host_ref/draw_sched_driver.cpp on a CPU.
//
// Launch length of the sampling phase.  Two things pull in opposite directions: a launch cannot end before its
// slowest wave (the tail is paid once per launch: long launches), and the dispatch order — heaviest chains first, lockstep
// neighbours with similar trees — is only as good as the prediction of a chain's work, which on heavy-tailed targets is its
// work in the launch just finished and fades within tens of transitions (short launches).  Measured whole sampling phase,
// every launch ordered by the work of the one before it: cfg3 (funnel) 250 / 62 / 16 / 8 / 4 per launch 1.83 / 2.06 / 2.42 /
// 2.56 / 2.73e9 leapfrog/s (one launch of 1 000 ordered by step size: 1.69e9); cfg2 (iso Gaussian) 250 / 64 / 16 / 8 2.94 /
// 2.89 / 2.80 / 2.58e9.  Neither the imbalance nor the launch-to-launch correlation at one length separates the two cases
// ahead of time, so the engine MEASURES: starting from 32 it times groups of launches (>= 64 transitions: leapfrogs of the
// group ÷ wall time, the stream synchronised at both ends — only while it searches), halves while that gains > 2 %; if the
// first halving does not, the tails decide and it takes the longest launch unless that loses > 1.5 % (then one doubling
// at a time from the start length).  Then it stays at the best length, asynchronous again (cfg3 settles at 4, cfg2 at 256).  The
// length is kept until the step sizes change.  AHMC_NUTS_DRAW_BATCH=n fixes it; AHMC_NUTS_SCHED=0 = one length for all
// (AHMC_INFO_NUTS_BATCH), as before round 4.  The chains do not depend on any of it (tests/test_pipeline_parity.py).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace ahmc {

// The environment switches of the sampling phase's launches, read once per ahmc_sample / ahmc_sample_from call (the tests toggle
// them between calls).
struct DrawEnv {
  int64_t draw_batch = 0;      // AHMC_NUTS_DRAW_BATCH=n > 0: every launch n transitions (split evenly), no search
  bool sched = true;           // AHMC_NUTS_SCHED=0: no search, one length for all (AHMC_INFO_NUTS_BATCH)
  // AHMC_NUTS_ORDER_REFRESH (default on since round 4; =0: from the run's totals) and not AHMC_NUTS_NO_ORDER: the dispatch order of
  // every launch from the work of the launch BEFORE it alone
  bool order_refresh = true;
  // AHMC_NUTS_FIRST_BATCH=n (experiments; default off): a short first launch while the dispatch order is still the one by
  // step size, so that everything after it is scheduled by measured work
  int first_batch = 0;
};

inline DrawEnv read_draw_env() {
  DrawEnv e;
  if (const char* s = std::getenv("AHMC_NUTS_DRAW_BATCH")) e.draw_batch = std::atoll(s);
  if (const char* s = std::getenv("AHMC_NUTS_SCHED")) e.sched = std::atoi(s) != 0;
  const char* orf = std::getenv("AHMC_NUTS_ORDER_REFRESH");
  e.order_refresh = (orf ? std::atoi(orf) != 0 : true) && !std::getenv("AHMC_NUTS_NO_ORDER");
  if (const char* s = std::getenv("AHMC_NUTS_FIRST_BATCH")) e.first_batch = std::atoi(s);
  return e;
}

// The state of the search.  A length is timed over a GROUP of launches (>= SCHED_GROUP transitions, one host synchronisation at
// each end).  Reset (invalidate_schedule) whenever the step sizes, the metric or the target change: the trees change with them.
struct DrawSched {
  static constexpr int64_t SCHED_MIN = 4, SCHED_START = 32, SCHED_GROUP = 64;
  static constexpr double GAIN_DOWN = 1.02;   // a shorter launch is taken if it gains more than 2 %
  static constexpr double KEEP_UP = 0.985;    // a longer one unless it loses more than 1.5 %

  // what the NEXT timed group tries (the numbers are what AHMC_DEBUG prints)
  enum Phase : int {
    FRESH = 0,    // nothing measured yet: the start length, min(SCHED_START, batch)
    SHORTER = 1,  // the start length is measured: its shorter neighbour, half of it
    DOWN = 2,     // halving gained: half again, while that gains and stays >= SCHED_MIN
    LONGEST = 3,  // the first halving did not gain (or there is nothing shorter): the tails decide, so the longest launch, `batch`
    SETTLED = 4,  // no more groups: every launch best_len (split evenly)
    UP = 5,       // the longest launch lost: one doubling at a time from the start length, while that does not lose
  };

  int phase = FRESH;
  int64_t len = 0, best_len = 0;  // the length the next step of the search starts from / the best one measured
  double best_thr = 0;            // its throughput
  bool primed = false;            // one unmeasured launch has put the dispatch order on measured work
  int64_t g_len = 0;              // the group being timed: its launch length,
  int g_left = 0;                 //   and how many of its launches are still to come

  struct Plan {
    int64_t k;     // transitions of the next launch
    bool probing;  // it belongs to a group that is being timed
    bool begins;   // … and is its first launch: the caller snapshots the work counters, empties the stream and starts the clock
    bool ends;     // … and is its last one: the caller measures after it and calls close_group
  };

  // a timed group of launches never spans two calls (the host time between them would be in its interval)
  void drop_group() { g_left = 0; }

  // (split the remaining transitions evenly: 50 = 13+13+12+12, not 16+16+16+2 — a short last batch would pay the whole
  // tree-size tail for two transitions)
  static int64_t even_split(int64_t left, int64_t dbatch) {
    const int64_t nb_left = (left + dbatch - 1) / dbatch;
    return (left + nb_left - 1) / nb_left;
  }

  // Operation 1: the next launch, `left` transitions before the end of the run and at most `batch` per launch (nuts_batch).
  // `search`: AHMC_NUTS_SCHED is on and the order is refreshed from every launch's work.
  Plan plan(int64_t left, int64_t batch, int64_t draw_batch, bool search, int first_batch, bool order_from_work, bool eps_scalar) {
    Plan p{0, false, false, false};
    if (draw_batch <= 0 && search && phase != SETTLED && batch >= 2 * SCHED_MIN) {
      if (g_left > 0 && g_len > left) g_left = 0;   // (never a launch longer than what is left; a group an earlier call left
                                                    // unfinished was dropped at this call's entry)
      if (g_left > 0) {                        // inside a group
        p.k = g_len; p.probing = true;
      } else if (!primed && !order_from_work && left >= 4 * SCHED_START) {
        p.k = 2 * SCHED_MIN; primed = true;    // (untimed: the first launch of a run is still ordered by step size)
      } else {
        const int64_t L = phase == FRESH ? std::min<int64_t>(SCHED_START, batch)
                        : phase == LONGEST ? batch                     // shorter did not pay: the tails decide, so the longest launch next
                        : phase == UP ? std::min<int64_t>(len * 2, batch)   // … and only if THAT loses, up one doubling at a time
                        : std::max<int64_t>(len / 2, SCHED_MIN);   // SHORTER: the shorter neighbour first; DOWN: further down
        const int64_t n_g = std::max<int64_t>(1, SCHED_GROUP / L);
        if (left >= L * n_g + L) {             // (worth timing, and something left to use the answer on)
          primed = true;
          g_len = L; g_left = (int)n_g;
          p.k = L; p.probing = true; p.begins = true;
        } else {
          p.k = even_split(left, best_len > 0 ? best_len : batch);   // too little left to learn from: the best length known
        }
      }
    } else {
      p.k = even_split(left, draw_batch > 0 ? draw_batch : (phase == SETTLED && search ? best_len : batch));
    }
    if (first_batch >= 4 && !order_from_work && !eps_scalar && left > 2 * (int64_t)first_batch && !p.probing) p.k = std::min<int64_t>(p.k, first_batch);
    p.ends = p.probing && g_left == 1;
    return p;
  }

  // after a launch of a timed group (Plan::probing)
  void timed_launch_done() { --g_left; }

  // Operation 2: the group of launches of `k` transitions that just ended ran at `thr` leapfrog/s.
  void close_group(int64_t k, double thr, int64_t batch) {
    if (phase == FRESH) { best_len = len = k; best_thr = thr; phase = k / 2 >= SCHED_MIN ? SHORTER : LONGEST; }
    else if (phase == SHORTER || phase == DOWN) {  // tried the shorter neighbour of the best
      if (thr > best_thr * GAIN_DOWN) {
        best_len = len = k; best_thr = thr;
        phase = k / 2 >= SCHED_MIN ? DOWN : SETTLED;
      } else if (phase == SHORTER) { len = best_len; phase = best_len * 2 <= batch ? LONGEST : SETTLED; }  // shorter does not pay: look the other way
      else phase = SETTLED;
    } else if (phase == LONGEST) {                 // tried the longest launch
      if (thr >= best_thr * KEEP_UP) { best_len = len = k; best_thr = std::max(best_thr, thr); phase = SETTLED; }
      else phase = best_len * 4 <= batch ? UP : SETTLED;   // (something between the start length and the longest is left to try)
    } else if (phase == UP) {                      // tried the longer neighbour
      if (thr >= best_thr * KEEP_UP) {
        best_len = len = k; best_thr = std::max(best_thr, thr);
        phase = k * 4 <= batch ? UP : SETTLED;
      } else phase = SETTLED;
    }
  }
};

}  // namespace ahmc
