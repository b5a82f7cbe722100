// ahmc_sample_host.hpp — the host side of ahmc_sample / ahmc_sample_from: the loop over transitions (sample_run), its four routes
// (batched draws, fused warm-up, dense StepSizeAdaptor warm-up, one transition at a time), the two-slot pipe that takes kept draws
// to a host buffer, and the momentum normals of a k_nuts launch (normals_for_launch / prefetch_next_normals, called by
// nuts_transition).  Included by ahmc_api.hip; the launch-length controller is ahmc_draw_sched.hpp.

// ---- the momentum normals of a k_nuts launch ----
template <class T>
unsigned normals_grid(const Ctx<T>* c, int64_t n) {
  const int64_t pairs = ((c->D + 1) / 2) * c->N * n;
  return (unsigned)std::min<int64_t>((pairs + 255) / 256, (int64_t)c->n_cu * 32);
}

// standard normals of the n_trans momentum refreshes (rand_momentum, src/metric.jl:290-309) in c->znorm: already made beside the
// launch before (prefetch_next_normals), in its tail (tail_normals_plan), or made now
template <class T>
int normals_for_launch(Ctx<T>* c, const KP<T>& p, int n_trans) {
  const size_t need = (size_t)n_trans * (size_t)c->D * (size_t)c->N;
  auto& np = c->npre;
  const bool hit = np.valid && np.iter == c->iteration && np.n >= n_trans && np.k0 == (uint64_t)p.k0 && np.k1 == (uint64_t)p.k1 &&
                   np.chain_offset == (uint64_t)p.chain_offset && np.chain_stride == (uint64_t)p.chain_stride && c->znorm2_elems >= need;
  np.valid = false;   // (used or stale: either way the buffer's content is spent)
  if (hit) {
    // (made by the waves behind the launch before, on c->stream itself: this launch is ordered behind them already)
    if (!np.in_tail) { HIPCHK(hipStreamWaitEvent(c->stream, c->ev_norm_ready, 0)); c->z2_norm_stream_busy = false; }
    std::swap(c->znorm, c->znorm2);
    std::swap(c->znorm_elems, c->znorm2_elems);
    HIPCHK(hipEventRecord(c->ev_z2_free, c->stream));   // everything that read the buffer that is now znorm2 lies before this point
    c->z2_has_reader = true;
    (np.in_tail ? c->norm_tail_hits : c->norm_prefetch_hits) += 1;
  } else {
    if (need > c->znorm_elems) {
      if (c->znorm) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->znorm)); }
      c->znorm = nullptr;
      HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->znorm), need * sizeof(T)));
      c->znorm_elems = need;
    }
    hipLaunchKernelGGL((k_normals<T>), dim3(normals_grid(c, n_trans)), dim3(256), 0, c->stream, p, c->znorm, n_trans, (uint32_t)RNG_MOMENTUM);
    HIPCHK(hipGetLastError());
  }
  return AHMC_OK;
}

// ---- the second normals buffer, at least `need2` elements: both ways of making the next launch's normals ahead of time write it ----
// Out of memory is not an error: `on` (the caller's switch for this context) goes to 0 and the caller's path is off from then on.
template <class T>
int second_normals_buffer(Ctx<T>* c, size_t need2, int& on) {
  if (!c->ev_z2_free) {
    HIPCHK(hipEventCreateWithFlags(&c->ev_norm_ready, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_z2_free, hipEventDisableTiming));
  }
  if (need2 <= c->znorm2_elems) return AHMC_OK;
  // a second buffer only where the device has room to spare (the draws of a run, another context): 2x its size must be free
  size_t free_b = 0, total_b = 0;
  const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b + c->znorm2_elems * sizeof(T) >= 2 * need2 * sizeof(T);
  (void)hipGetLastError();
  if (room) {
    if (c->znorm2) {
      HIPCHK(hipStreamSynchronize(c->stream));
      if (c->stream_norm) HIPCHK(hipStreamSynchronize(c->stream_norm));
      HIPCHK(hipFree(c->znorm2));
      c->z2_has_reader = false;
      c->z2_norm_stream_busy = false;
      c->npre.valid = false;
    }
    c->znorm2 = nullptr;
    c->znorm2_elems = 0;
    if (hipMalloc(reinterpret_cast<void**>(&c->znorm2), need2 * sizeof(T)) == hipSuccess) c->znorm2_elems = need2;
    else { (void)hipGetLastError(); c->znorm2 = nullptr; on = 0; }
  } else if (!c->znorm2) {
    on = 0;
  }
  return AHMC_OK;
}

#ifndef AHMC_NORMALS_TAIL_DEFAULT
#define AHMC_NORMALS_TAIL_DEFAULT 1
#endif
// AHMC_NORMALS_TAIL (read per call): 0 off; 1 where the second stream is declined for size alone; 2 every launch length (tests, A/B runs)
inline int normals_tail_mode() {
  const char* e = getenv("AHMC_NORMALS_TAIL");
  const int m = e ? atoi(e) : AHMC_NORMALS_TAIL_DEFAULT;
  return m < 0 ? 0 : (m > 2 ? 2 : m);
}
inline size_t normals_prefetch_max_bytes() {
  return getenv("AHMC_NORMALS_PREFETCH_MAX_MB") ? (size_t)atoll(getenv("AHMC_NORMALS_PREFETCH_MAX_MB")) << 20 : (size_t)2 << 30;
}
// does a launch whose successor has `hint` transitions make that successor's normals in its own tail?  (k_nuts, G = 64, MODE 0 / 3:
// "tail normals" in ahmc_kernels.hpp.)  Mode 1 takes exactly the launches the second stream declines for their size.
template <class T>
bool tail_normals_applies(const Ctx<T>* c, int64_t hint, double refresh_alpha) {
  const int mode = normals_tail_mode();
  if (mode == 0 || c->norm_tail == 0 || c->G != 64 || hint <= 0 || refresh_alpha != 0) return false;
  if (mode == 2) return true;
  if (getenv("AHMC_NORMALS_PREFETCH") && atoi(getenv("AHMC_NORMALS_PREFETCH")) == 0) return false;
  return (size_t)hint * (size_t)c->D * (size_t)c->N * sizeof(T) > normals_prefetch_max_bytes();
}

// ---- the normals of the launch that follows, in the TAIL of the one about to be enqueued ----
// Fills p.tail_*: `tail_waves` single-wave workgroups behind the chain workgroups, `AHMC_NORMALS_TAIL_ROWS` rows each (a row = one
// transition of one chain), writing the second buffer.  The hardware deals workgroups in block order, so they start when the last chain
// has started and fill the wave slots that empty out while the launch waits for its slowest chains (measured: profiles/r8_experiments.md).
template <class T>
int tail_normals_plan(Ctx<T>* c, KP<T>& p, int64_t hint, int n_trans) {
  const size_t need2 = (size_t)hint * (size_t)c->D * (size_t)c->N;
  if (c->norm_tail < 0) c->norm_tail = 1;
  int rc = second_normals_buffer(c, need2, c->norm_tail);
  if (rc) return rc;
  if (c->norm_tail != 1 || !c->znorm2 || need2 > c->znorm2_elems) return AHMC_OK;
  // a k_normals of the second stream may still be writing the buffer (its launch was never consumed): behind it
  if (c->z2_norm_stream_busy) { HIPCHK(hipStreamWaitEvent(c->stream, c->ev_norm_ready, 0)); c->z2_norm_stream_busy = false; }
  const int rows_env = getenv("AHMC_NORMALS_TAIL_ROWS") ? atoi(getenv("AHMC_NORMALS_TAIL_ROWS")) : 0;
  const int64_t rows = hint * c->N, per_wave = rows_env > 0 ? rows_env : 64;
  p.tail_out = c->znorm2;
  p.tail_n_trans = (int)hint;
  p.tail_iteration = (uint32_t)(c->iteration + (uint64_t)n_trans);
  p.tail_rows = (int)per_wave;
  p.tail_waves = (unsigned int)((rows + per_wave - 1) / per_wave);
  return AHMC_OK;
}
template <class T>
bool tail_normals_planned(const KP<T>& p) {
  return p.tail_waves != 0;
}
// after that launch: what the second buffer will hold, and that the stream is still writing it (a later k_normals of the second stream waits)
template <class T>
int tail_normals_done(Ctx<T>* c, const KP<T>& p) {
  HIPCHK(hipEventRecord(c->ev_z2_free, c->stream));
  c->z2_has_reader = true;
  c->npre.valid = true;
  c->npre.in_tail = true;
  c->npre.iter = c->iteration; c->npre.n = p.tail_n_trans;
  c->npre.k0 = (uint64_t)p.k0; c->npre.k1 = (uint64_t)p.k1; c->npre.chain_offset = (uint64_t)p.chain_offset; c->npre.chain_stride = (uint64_t)p.chain_stride;
  return AHMC_OK;
}

// ---- the normals of the launch that follows (`hint` transitions, from c->iteration on), beside the one just enqueued ----
// Measured (profiles/r6_experiments.md r6n): cfg3's 4-transition launches gain 6 % in the sampling phase (3.20 -> 3.40e9: the 0.1 ms of
// k_normals and its launch gap no longer sit between two 6 ms launches); cfg2's 256-transition launches lose 0.4 % (a 5.7 ms k_normals beside
// a VALU-bound k_nuts takes what it gives) and cfg5's 32 are unchanged — so only launches whose normals are at most 2 GiB are prefetched.
template <class T>
int prefetch_next_normals(Ctx<T>* c, const KP<T>& p, int64_t hint, double refresh_alpha) {
  const size_t prefetch_max_bytes = normals_prefetch_max_bytes();
  if (!(hint > 0 && refresh_alpha == 0 && (size_t)hint * (size_t)c->D * (size_t)c->N * sizeof(T) <= prefetch_max_bytes)) return AHMC_OK;
  if (c->norm_prefetch < 0) c->norm_prefetch = (getenv("AHMC_NORMALS_PREFETCH") && atoi(getenv("AHMC_NORMALS_PREFETCH")) == 0) ? 0 : 1;
  const size_t need2 = (size_t)hint * (size_t)c->D * (size_t)c->N;
  if (c->norm_prefetch == 1) {
    int rc = second_normals_buffer(c, need2, c->norm_prefetch);
    if (rc) return rc;
  }
  if (c->norm_prefetch == 1 && c->znorm2 && need2 <= c->znorm2_elems) {
    if (!c->stream_norm) HIPCHK(hipStreamCreateWithFlags(&c->stream_norm, hipStreamNonBlocking));
    if (c->z2_has_reader) HIPCHK(hipStreamWaitEvent(c->stream_norm, c->ev_z2_free, 0));
    KP<T> p2 = p;
    p2.iteration = (uint32_t)c->iteration;   // (make_kp's field: the launch that follows starts here)
    hipLaunchKernelGGL((k_normals<T>), dim3(normals_grid(c, hint)), dim3(256), 0, c->stream_norm, p2, c->znorm2, (int)hint, (uint32_t)RNG_MOMENTUM);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev_norm_ready, c->stream_norm));
    c->z2_norm_stream_busy = true;
    c->npre.valid = true;
    c->npre.in_tail = false;
    c->npre.iter = c->iteration; c->npre.n = hint;
    c->npre.k0 = (uint64_t)p.k0; c->npre.k1 = (uint64_t)p.k1; c->npre.chain_offset = (uint64_t)p.chain_offset; c->npre.chain_stride = (uint64_t)p.chain_stride;
  }
  return AHMC_OK;
}

// ---- ahmc_sample(samples_out = host buffer): the two-slot pipe ----
// k_nuts writes a batch's draws into one of two device stages (Ctx::stage); the D2H copy of one batch runs on copy_stream while
// k_nuts fills the other stage.  The events, streams and buffers are the context's; this is one call's position in the pipe.
template <class T>
struct DrawStage {
  int64_t n_staged = 0;
  T* pend_dst = nullptr;   // the batch whose draws are still in a stage: where they go, which stage, how many bytes
  int pend_slot = 0;
  size_t pend_bytes = 0;

  int slot() const { return (int)(n_staged & 1); }

  // the next stage, at least `need` elements, not in use by a copy any more (device-side wait: the next k_nuts that writes it is
  // ordered after the D2H copy that reads it)
  int acquire(Ctx<T>* c, size_t need, T** dev_dst) {
    const int s = slot();
    if (!c->copy_stream) {
      HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
      for (int e = 0; e < 2; ++e) {
        HIPCHK(hipEventCreateWithFlags(&c->stage_ready[e], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c->stage_free[e], hipEventDisableTiming));
      }
    }
    if (need > c->stage_elems[s]) {
      HIPCHK(hipStreamSynchronize(c->copy_stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      if (c->stage[s]) HIPCHK(hipFree(c->stage[s]));
      c->stage[s] = nullptr;
      c->stage_elems[s] = 0;
      HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->stage[s]), need * sizeof(T)));
      c->stage_elems[s] = need;
      c->stage_busy[s] = false;
    } else if (c->stage_busy[s]) {
      HIPCHK(hipStreamWaitEvent(c->stream, c->stage_free[s], 0));
      c->stage_busy[s] = false;
    }
    *dev_dst = c->stage[s];
    return AHMC_OK;
  }

  int flush(Ctx<T>* c) {
    if (!pend_dst) return AHMC_OK;
    HIPCHK(hipStreamWaitEvent(c->copy_stream, c->stage_ready[pend_slot], 0));
    HIPCHK(hipMemcpyAsync(pend_dst, c->stage[pend_slot], pend_bytes, hipMemcpyDeviceToHost, c->copy_stream));
    HIPCHK(hipEventRecord(c->stage_free[pend_slot], c->copy_stream));
    c->stage_busy[pend_slot] = true;
    pend_dst = nullptr;
    return AHMC_OK;
  }

  // after the launch that filled the acquired stage: its `bytes` go to `dst` once the NEXT launch is enqueued
  int submit(Ctx<T>* c, T* dst, size_t bytes) {
    const int s = slot();
    HIPCHK(hipEventRecord(c->stage_ready[s], c->stream));
    // the PREVIOUS batch's draws go to the host while this batch computes (a copy to pageable memory blocks the
    // calling thread, so it is issued after this batch's launch, not before)
    int rc = flush(c);
    if (rc) return rc;
    pend_dst = dst; pend_slot = s; pend_bytes = bytes;
    ++n_staged;
    return AHMC_OK;
  }

  // last staged batch; the context's stream then waits for the copies, so ahmc_sync covers them
  int drain(Ctx<T>* c) {
    int rc = flush(c);
    if (rc) return rc;
    for (int s = 0; s < 2; ++s)
      if (c->stage_busy[s]) {
        HIPCHK(hipStreamWaitEvent(c->stream, c->stage_free[s], 0));
        c->stage_busy[s] = false;
      }
    return AHMC_OK;
  }
};

// what one ahmc_sample / ahmc_sample_from call was asked for, and what it found out once at its entry
template <class T>
struct SampleCall {
  const ahmc_kernel_cfg* cfg;
  int64_t n_samples, n_adapts;
  bool drop_warmup;
  T* so;                // samples_out (may be null)
  bool so_on_device;    // can k_nuts write the kept draws itself?  (device buffer, or none requested)
  int64_t batch;        // transitions per launch at most (nuts_batch, the reserved normals)
  DrawEnv env;
  DrawStage<T> stage;

  // where the draw of transition i goes in samples_out
  T* dst(const Ctx<T>* c, int64_t i) const {
    const int64_t j = i - (drop_warmup ? n_adapts : 0);
    return so + (size_t)(j - 1) * c->D * c->N;
  }
};

template <class T>
int sample_check(Ctx<T>* c, const ahmc_kernel_cfg* cfg, int64_t i_first, int64_t n_adapts, bool drop_warmup) {
  if (!cfg) return fail(c, AHMC_ERR_ARGUMENT, "sample: cfg is NULL");
  if (i_first < 1) return fail(c, AHMC_ERR_ARGUMENT, "sample_from: i_first must be >= 1");
  if (!c->have_point) return fail(c, AHMC_ERR_STATE, "sample before set_position");
  if (drop_warmup && c->adapt_kind == AHMC_ADAPT_NONE)
    return fail(c, AHMC_ERR_ARGUMENT, "Cannot drop warmup samples if there is no adaptation phase.");  // src/sampler.jl:172
  if (c->lr.on && c->adapt_kind != AHMC_ADAPT_NONE && c->adapt_kind != AHMC_ADAPT_STEPSIZE && c->metric_kind != AHMC_METRIC_RANK_UPDATE_CTX)
    return fail(c, AHMC_ERR_UNSUPPORTED, "sample: the low-rank adaptor fits a RankUpdateEuclideanMetric and the context's metric was replaced by another kind: "
                                         "set up an adaptor again");
  if (c->metric_kind == AHMC_METRIC_RANK_UPDATE_CTX && c->adapt_kind != AHMC_ADAPT_NONE && c->adapt_kind != AHMC_ADAPT_STEPSIZE && !c->lr.on)
    return fail(c, AHMC_ERR_UNSUPPORTED, "sample: RankUpdateEuclideanMetric has no mass-matrix adaptor (the adaptor was set up for another metric)");
  // a resumed run must continue where the restored state stopped: a Stan adaptor counts its own calls (state.i,
  // stan_adaptor.jl:137-159), so while it is adapting the absolute iteration is known and a mismatch is an error rather
  // than a silently wrong window schedule
  if (i_first > 1 && c->adapt_kind == AHMC_ADAPT_STAN && c->adapting && i_first <= n_adapts && c->stan_i != i_first - 1)
    return fail(c, AHMC_ERR_STATE, "sample_from: i_first = " + std::to_string(i_first) + " but the adaptor has seen " + std::to_string(c->stan_i) +
                                       " iterations (restore the checkpoint taken after iteration i_first - 1: ahmc_set_adaptor_state)");
  return AHMC_OK;
}

// Dispatch order by measured work: a better predictor of a chain's tree sizes than its step size is what it
// actually did — Σ n_steps per chain of the previous sampling call (still in the accumulators here) or of
// this call's first batch.  Counting sort on the stream, no host synchronisation.
// (Round 3, measured and NOT taken: using the counts of the call before even when the ϵ order has been invalidated — i.e. the
// warm-up's Σ n_steps for the first launch of the draws, and then for all of them —: cfg2 draws 2.97e9 -> 2.41e9, cfg3
// 1.70e9 -> 1.58e9 (one launch: a clean comparison; cfg2's figure also contains that its later launches no longer switched to
// the first launch's counts).  What a chain did while it was still adapting predicts its sampling work worse than its final ϵ.)
template <class T>
int order_by_work(Ctx<T>* c, const ahmc_kernel_cfg* cfg, bool refresh) {
  if (!cfg->nuts || dense_engine(c) || !c->order_valid || (c->order_from_work && !refresh) || c->acc_ntrans < 4) return AHMC_OK;
  int rc = build_order(c, (int)std::min<int64_t>(c->acc_ntrans, 1 << 20));
  if (!rc) c->order_from_work = true;
  return rc;
}

// One batched launch of the sampling phase, from transition i on: chains are independent and nothing is adapted any more, so a
// batch of transitions runs per launch (no per-transition barrier; see the note on tree-size tails in ahmc_nuts.hpp).  How many
// is the controller's decision (ahmc_draw_sched.hpp); `k` returns it.
template <class T>
int sample_draws_launch(Ctx<T>* c, SampleCall<T>& s, int64_t i, int64_t& k) {
  const ahmc_kernel_cfg* cfg = s.cfg;
  // the dispatch order of every launch from the work of the launch BEFORE it alone
  const bool order_refresh = s.env.order_refresh && !dense_engine(c) && !c->eps_scalar;
  const int64_t left = s.n_samples - i + 1;
  auto& sc = c->sched;
  const DrawSched::Plan pl = sc.plan(left, s.batch, s.env.draw_batch, s.env.sched && order_refresh, s.env.first_batch, c->order_from_work, c->eps_scalar);
  k = pl.k;
  if (pl.begins) {
    if (!c->work_grp) HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->work_grp), sizeof(long long) * (size_t)c->N));
    if (!c->work_sum) HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->work_sum), sizeof(long long)));
    HIPCHK(hipMemcpyAsync(c->work_grp, c->acc_nsteps, sizeof(long long) * (size_t)c->N, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // (the clock starts on an empty stream)
    c->sched_t0 = std::chrono::steady_clock::now();
  }
  T* dst = s.so ? s.dst(c, i) : nullptr;
  T* dev_dst = dst;
  const bool via_stage = s.so && !s.so_on_device;
  if (via_stage) {  // host buffer: the kernel writes the batch's draws into a device stage
    int rc1 = s.stage.acquire(c, (size_t)k * c->D * c->N, &dev_dst);
    if (rc1) return rc1;
  }
  if (order_refresh) {
    if (!c->work_prev) {
      HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->work_prev), sizeof(long long) * (size_t)c->N));
      HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->work_last), sizeof(long long) * (size_t)c->N));
    }
    HIPCHK(hipMemcpyAsync(c->work_prev, c->acc_nsteps, sizeof(long long) * (size_t)c->N, hipMemcpyDeviceToDevice, c->stream));
  }
  // (the launch after this one: the same length unless a timed group ends here or the run does — its normals are made beside this one)
  c->norm_hint = (left > k && !pl.ends) ? std::min<int64_t>(k, left - k) : 0;
  int rc = nuts_transition(c, cfg->max_depth, cfg->delta_max, cfg->criterion, cfg->sampler, cfg->refresh_alpha, true,
                           (int)k, dev_dst);
  if (rc) return rc;
  if (order_refresh && k >= 2) {
    hipLaunchKernelGGL(k_work_since, dim3((unsigned)((c->N + 255) / 256)), dim3(256), 0, c->stream, c->acc_nsteps, c->work_prev, c->work_last, (int64_t)c->N);
    HIPCHK(hipGetLastError());
    rc = build_order(c, (int)k, c->work_last);
    if (rc) return rc;
    c->order_valid = true;
    c->order_from_work = true;
  }
  if (pl.probing) sc.timed_launch_done();
  if (pl.ends) {
    // leapfrogs of the group ÷ its wall time (everything it needed: normals, both passes, the re-sorts)
    HIPCHK(hipMemsetAsync(c->work_sum, 0, sizeof(long long), c->stream));
    hipLaunchKernelGGL(k_work_sum, dim3(64), dim3(256), 0, c->stream, c->acc_nsteps, c->work_grp, c->work_sum, (int64_t)c->N);
    HIPCHK(hipGetLastError());
    long long w = 0;
    HIPCHK(hipMemcpyAsync(&w, c->work_sum, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - c->sched_t0).count();
    const double thr = dt > 0 ? (double)w / dt : 0.0;
    static const bool dbg_s = getenv("AHMC_DEBUG") != nullptr;
    if (dbg_s) fprintf(stderr, "[ahmc] sched: phase %d, %lld transitions per launch: %.4e leapfrog/s (best so far %lld: %.4e)\n", sc.phase, (long long)k, thr, (long long)sc.best_len, sc.best_thr);
    sc.close_group(k, thr, s.batch);
    if (dbg_s && sc.phase == DrawSched::SETTLED) fprintf(stderr, "[ahmc] sched: settled at %lld transitions per launch\n", (long long)sc.best_len);
  }
  if (via_stage) {
    rc = s.stage.submit(c, dst, sizeof(T) * c->D * c->N * (size_t)k);
    if (rc) return rc;
  }
  c->acc_ntrans += k;
  return order_by_work(c, cfg, false);  // (first batch of a fresh chain set: from now on schedule by measured work)
}

// AHMC_ADAPT_FUSED=0: every adapting transition a launch of its own (both batched warm-up routes off)
inline bool adapt_fused() {
  static const bool on = getenv("AHMC_ADAPT_FUSED") ? atoi(getenv("AHMC_ADAPT_FUSED")) != 0 : true;
  return on;
}

// Can the adapting transitions run as fused launches (k_nuts MODE 3: adapt! inside the kernel)?
template <class T>
bool warmup_fused_applies(const Ctx<T>* c, const SampleCall<T>& s, bool keep) {
  const ahmc_kernel_cfg* cfg = s.cfg;
  return adapt_fused() && cfg->nuts && cfg->sampler == AHMC_TS_MULTINOMIAL && cfg->criterion == AHMC_TC_GENERALISED &&
         !dense_engine(c) && c->integ_kind != AHMC_INTEGRATOR_TEMPERED && c->target_kind != AHMC_TARGET_EXTERNAL &&
         (!s.so || !keep || s.so_on_device) &&
         !(c->var_estimator == AHMC_VAR_POOLED && c->adapt_kind != AHMC_ADAPT_STAN && c->adapt_kind != AHMC_ADAPT_STEPSIZE);
}

// warm-up in batches too: adapt! runs inside the kernel (k_nuts MODE 3), no per-transition launch
// (round 4, measured and dropped: the warm-up in launches of 8 / 32 / 64 transitions, each ordered by the work of the one before
// it — cfg3 1.98 / 2.00e9 against 1.98e9 for one launch ordered by step size, cfg2 2.27e9 against 2.39e9: while the step
// sizes still move a launch's work does not predict the next one's any better than ϵ does, and every launch pays its tail.
// Nor does a PILOT: the first 50 / 100 / 200 transitions as a launch of their own and the rest ordered by the work measured
// in it — cfg3 warm-up 1.99 / 1.96 / 1.90e9 against 2.05e9, cfg2 2.54e9 against 2.57e9.  The one launch's wave timeline
// (profiles/r4_cfg3_wave_timeline_warmup_launch.json): fill 0.65, the longest wave 0.48 of the launch)
template <class T>
int sample_warmup_fused(Ctx<T>* c, SampleCall<T>& s, int64_t i, bool keep, int64_t& k) {
  const int64_t n_adapts = s.n_adapts;
  const int64_t left = std::min(n_adapts, s.n_samples) - i + 1;  // (a run may end mid-warm-up)
  k = DrawSched::even_split(left, s.batch);
  if (c->var_estimator == AHMC_VAR_POOLED && c->adapt_kind == AHMC_ADAPT_STAN && c->metric_kind == AHMC_METRIC_DIAG) {
    // the pooled estimator couples the chains at the window ends: a batch stops there (one reduction, and with a
    // communicator one all-gather, per window — not per transition)
    if (i == 1 || c->windows_n_adapts != n_adapts) {
      c->windows = stan_windows(c->stan_init, c->stan_term, c->stan_window, n_adapts);
      c->windows_n_adapts = n_adapts;
    }
    for (int64_t sp : c->windows.splits) {
      const int64_t stan_at = c->stan_i + 1;  // StanHMCAdaptor.state.i of transition i
      if (sp >= stan_at) { k = std::min<int64_t>(k, sp - stan_at + 1); break; }
    }
  }
  T* dst = (s.so && keep) ? s.dst(c, i) : nullptr;
  // (round 4, measured and dropped: the warm-up as 2 / 4 interleaved groups of chains, each a sequence of launches of 8 … 125
  // transitions on its own stream, so that the slots one group's launch leaves empty at its end would be filled by the others'
  // — cfg3 warm-up 1.81 / 1.10e9 (launches of 32) against 1.94e9 for the one launch, cfg2 2.31–2.38e9 against 2.59e9: the
  // queues do not interleave at workgroup granularity, a group's launch only under-fills the chip)
  {
    const int64_t after = std::min(n_adapts, s.n_samples) - (i + k) + 1;   // adapting transitions left after this launch
    c->norm_hint = after > 0 ? std::min<int64_t>(k, after) : 0;
  }
  int rc = nuts_adapt_batch(c, s.cfg, (int)k, i, n_adapts, keep, dst);
  if (rc) return rc;
  if (keep) c->acc_ntrans += k;
  return AHMC_OK;
}

template <class T>
bool warmup_dense_applies(const Ctx<T>* c, const SampleCall<T>& s, bool keep) {
  const ahmc_kernel_cfg* cfg = s.cfg;
  return adapt_fused() && cfg->nuts && dense_engine(c) && c->adapt_kind == AHMC_ADAPT_STEPSIZE &&
         (cfg->sampler == AHMC_TS_MULTINOMIAL || cfg->sampler == AHMC_TS_SLICE) &&
         cfg->refresh_alpha == 0 && c->target_kind != AHMC_TARGET_EXTERNAL &&
         (!s.so || !keep || s.so_on_device);
}

// dense engine, StepSizeAdaptor: the warm-up in batches too — every chain adapts its own ϵ at the end of each of its
// transitions inside the tree kernel and goes on, instead of all chains waiting for the longest tree of every transition
template <class T>
int sample_warmup_dense(Ctx<T>* c, SampleCall<T>& s, int64_t i, bool keep, int64_t& k) {
  const ahmc_kernel_cfg* cfg = s.cfg;
  k = DrawSched::even_split(std::min(s.n_adapts, s.n_samples) - i + 1, s.batch);
  T* dst = (s.so && keep) ? s.dst(c, i) : nullptr;
  int rc = dn_nuts_transition(c, cfg->max_depth, cfg->delta_max, cfg->criterion, cfg->sampler, cfg->refresh_alpha, keep, (int)k, dst, i - 1, s.n_adapts);
  if (rc) return rc;
  c->eps_scalar = false;
  if (i + k - 1 >= s.n_adapts) c->adapting = false;
  if (keep) c->acc_ntrans += k;
  return AHMC_OK;
}

// everything else: one transition per launch, adapt! between two of them
template <class T>
int sample_one_transition(Ctx<T>* c, SampleCall<T>& s, int64_t i, bool keep) {
  const ahmc_kernel_cfg* cfg = s.cfg;
  int rc = cfg->nuts ? nuts_transition(c, cfg->max_depth, cfg->delta_max, cfg->criterion, cfg->sampler, cfg->refresh_alpha, keep)
                     : hmc_transition(c, cfg->L, cfg->lambda, cfg->sampler, cfg->refresh_alpha, keep);
  if (rc) return rc;
  rc = adapt(c, i, s.n_adapts);
  if (rc) return rc;
  if (keep) {
    c->acc_ntrans += 1;
    if (s.so) HIPCHK(hipMemcpyAsync(s.dst(c, i), c->th, sizeof(T) * c->D * c->N, hipMemcpyDefault, c->stream));
  }
  return AHMC_OK;
}

// ahmc_sample / ahmc_sample_from: transitions i_first .. n_samples (src/sampler.jl:182-228)
template <class T>
int sample_run(Ctx<T>* c, const ahmc_kernel_cfg* cfg, int64_t i_first, int64_t n_samples, int64_t n_adapts, bool drop_warmup, T* so) {
  int rc = sample_check(c, cfg, i_first, n_adapts, drop_warmup);
  if (rc) return rc;
  c->sched.drop_group();
  // the accumulators are reset at the first kept transition — unless the run is being RESUMED beyond it (ahmc_sample_from):
  // then they continue (a checkpoint carries them: ahmc_get/set_accum_state)
  bool reset_done = i_first > (drop_warmup ? n_adapts + 1 : 1);
  SampleCall<T> s{cfg, n_samples, n_adapts, drop_warmup, so, false, nuts_batch(c), read_draw_env(), {}};
  if (so) {
    hipPointerAttribute_t at;
    s.so_on_device = hipPointerGetAttributes(&at, so) == hipSuccess && at.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
  }
  if (cfg->nuts && !dense_engine(c) && c->target_kind != AHMC_TARGET_EXTERNAL && n_samples >= i_first) {
    // the normals of this call's longest launch (lazily, bounded by the call's own length; ahmc_sample_reserve does it ahead of time)
    rc = reserve_normals(c, std::min<int64_t>(s.batch, n_samples - i_first + 1));
    if (rc) return rc;
    if (c->znorm_cap_trans > 0) s.batch = std::min<int64_t>(s.batch, c->znorm_cap_trans);
  }
  rc = order_by_work(c, cfg, true);  // the previous call's counts are the freshest estimate there is
  if (rc) return rc;
  for (int64_t i = i_first; i <= n_samples;) {
    const bool keep = !drop_warmup || i > n_adapts;
    if (keep && !reset_done) {
      rc = reset_accum(c);
      if (rc) return rc;
      reset_done = true;
    }
    const bool adapting = c->adapt_kind != AHMC_ADAPT_NONE && i <= n_adapts;
    int64_t k = 1;
    if (cfg->nuts && !adapting && keep) rc = sample_draws_launch(c, s, i, k);
    else if (adapting && warmup_fused_applies(c, s, keep)) rc = sample_warmup_fused(c, s, i, keep, k);
    else if (adapting && warmup_dense_applies(c, s, keep)) rc = sample_warmup_dense(c, s, i, keep, k);
    else rc = sample_one_transition(c, s, i, keep);
    if (rc) return rc;
    i += k;
  }
  return s.stage.drain(c);
}
