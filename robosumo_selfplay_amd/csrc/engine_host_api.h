// engine_host_api.h -- the C ABI of an engine (include/sumo_hip.h): variant dispatch, sumo_create / destroy / dims / reset / step,
// then the settings, read-backs and state access (sumo_set_cfrc_mode .. sumo_stats).  Not in a shard object.
// A part of the sumo_engine.hip translation unit, not a stand-alone header: no includes of its own.

// kernel variants by nv (the factorisation is unrolled over a compile-time nv); the nine registered scenes have
// nv in {28, 32, 36, 40, 44}
template <class F>
static bool for_kernel_variant(int nv, F&& f) {
#define X(NVV) if (nv == NVV) { f(std::integral_constant<int, NVV>()); return true; }
  SUMO_FOR_NV(X)
#undef X
  return false;
}

// an env record of more than the 64 KB of LDS a launch gets without asking
template <int NV>
static int allow_large_lds(int bytes) {
  HIPCHK(hipFuncSetAttribute((const void*)sumo_step_kernel<NV>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  HIPCHK(hipFuncSetAttribute((const void*)sumo_reset_kernel<NV>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  HIPCHK(hipFuncSetAttribute((const void*)sumo_forward_kernel<NV>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  return 0;
}

// Every failure below returns through the unique_ptr: the engine and whatever it had allocated on the device go with it.
extern "C" int sumo_create(const void* model_blob, size_t nbytes, int num_envs, int device, sumo_handle_t* out) {
  if (!model_blob || !out || num_envs <= 0) FAIL(-1, "bad arguments");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) FAIL(-2, "no HIP device available: the engine has no CPU fallback");
  if (device < 0 || device >= ndev) FAIL(-3, "device %d out of range (%d devices)", device, ndev);
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<sumo_engine> E(new sumo_engine());
  E->device = device; E->N = num_envs;
  if (int rc = prepare_scene(*E, model_blob, nbytes, SCENE_CHECKED)) return rc;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if ((size_t)E->L.total_bytes > prop.sharedMemPerBlock && (size_t)E->L.total_bytes > 160 * 1024)
    FAIL(-5, "LDS need %d bytes exceeds the device limit", E->L.total_bytes);
  const sumo_model_t* m = &E->hm;
  HIPCHK(E->d_blob.upload(E->blob));
  HIPCHK(E->d_ai.upload(E->ai));
  HIPCHK(E->d_af.upload(E->af));
  HIPCHK(E->d_pic.upload(E->pic));
  HIPCHK(E->d_lanes.upload(E->lanes));
  HIPCHK(E->d_pair_rec.upload(E->pair_rec));
  HIPCHK(E->d_pair_bound.upload(E->pair_bound));
  {
    Params hp;
    hp.mdl = E->hm;   // the device view: the host view with its table bases inside the uploaded blob
    hp.mdl.ibase = (const int32_t*)(E->d_blob.get() + ((const char*)E->hm.ibase - E->blob.data()));
    hp.mdl.fbase = (const double*)(E->d_blob.get() + ((const char*)E->hm.fbase - E->blob.data()));
    hp.aux = E->aux; hp.aux.ai = E->d_ai; hp.aux.af = E->d_af; hp.aux.pic = E->d_pic;
    hp.L = E->L;
    hp.lanes = E->d_lanes; hp.pair_rec = E->d_pair_rec; hp.pair_bound = E->d_pair_bound;
    hp.adjust_z = 0.0;
    hp.grad_thresh = E->grad_thresh;
    HIPCHK(E->d_params.alloc(1));
    HIPCHK(hipMemcpy(E->d_params, &hp, sizeof(Params), hipMemcpyHostToDevice));
  }
  size_t N = (size_t)num_envs;
  HIPCHK(E->d_state.alloc(N * E->state_stride));
  HIPCHK(hipMemset(E->d_state, 0, N * E->state_stride * sizeof(double)));
  HIPCHK(E->d_counters.alloc(N * 4));
  HIPCHK(hipMemset(E->d_counters, 0, N * 4 * sizeof(int)));
  std::vector<uint64_t> seeds(N);
  for (size_t i = 0; i < N; i++) seeds[i] = i;
  HIPCHK(E->d_seeds.upload(seeds));
  HIPCHK(E->d_stats.alloc(48));
  HIPCHK(hipMemset(E->d_stats, 0, 48 * sizeof(unsigned long long)));
  {
    const char* sc = getenv("SUMO_SCHED");
    E->sched = !(sc && atoi(sc) == 0);
    HIPCHK(E->d_cost.alloc(2 * N));
    HIPCHK(E->d_cost_sorted.alloc(N));
    HIPCHK(E->d_perm.alloc(2 * N));
    std::vector<int> iota(N);
    for (size_t i = 0; i < N; i++) iota[i] = (int)i;
    HIPCHK(E->d_iota.upload(iota));
    HIPCHK(rocprim::radix_sort_pairs_desc(nullptr, E->sort_tmp_bytes, E->d_cost.get(), E->d_cost_sorted.get(), E->d_iota.get(), E->d_perm.get(), N,
                                          0, 16, (hipStream_t)0));
    HIPCHK(E->d_sort_tmp.alloc(E->sort_tmp_bytes ? E->sort_tmp_bytes : 16));
  }
  // qpos = qpos0 for every env until the first reset / set_state
  {
    std::vector<double> st(N * E->state_stride, 0.0);
    for (size_t e = 0; e < N; e++) memcpy(&st[e * E->state_stride], SUMO_F(m, qpos0), m->nq * sizeof(double));
    HIPCHK(hipMemcpy(E->d_state, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (E->L.total_bytes > 64 * 1024) {
    int rc = 0;
    for_kernel_variant(E->hm.nv, [&](auto nvc_) { rc = allow_large_lds<decltype(nvc_)::value>(E->L.total_bytes); });
    if (rc) return rc;
  }
  *out = E.release();
  return 0;
}

extern "C" int sumo_destroy(sumo_handle_t E) {
  if (!E) return 0;
  (void)hipSetDevice(E->device);
  delete E;   // its DevBuf members free the device memory
  return 0;
}

extern "C" int sumo_dims(sumo_handle_t E, int32_t* o) {
  if (!E || !o) FAIL(-1, "bad arguments");
  const sumo_model_t* m = &E->hm;
  int v[SUMO_NDIMS] = {m->nq, m->nv, m->nu, m->nbody, m->njnt, m->ngeom, m->npair, m->nagent, E->obs_stride, E->act_stride,
                       E->L.maxcon, E->L.maxefc, E->L.total_bytes, E->state_stride, E->L.jbcap, 0};
  memcpy(o, v, sizeof v);
  return 0;
}

// the variant an engine's step / rollout kernels run: f(NV, SL) with the static layouts <28, 1> (Ant vs Ant) and <44, 2> (Spider
// vs Spider) where sumo_create found one, else <nv, 0>
template <class F>
static bool for_engine_variant(const sumo_engine* E, F&& f) {
  if (E->static_layout == 1) { f(std::integral_constant<int, 28>(), std::integral_constant<int, 1>()); return true; }
  if (E->static_layout == 2) { f(std::integral_constant<int, 44>(), std::integral_constant<int, 2>()); return true; }
  return for_kernel_variant(E->hm.nv, [&](auto nvc_) { f(nvc_, std::integral_constant<int, 0>()); });
}
#define SUMO_DISPATCH(KERNEL, E, stream, args) SUMO_DISPATCH_N(KERNEL, E, stream, args, (E)->N)
#define SUMO_DISPATCH_N(KERNEL, E, stream, args, nblocks)                                                   \
  do {                                                                                                       \
    dim3 g_(nblocks), b_(WAVE);                                                                              \
    size_t lds_ = (size_t)(E)->L.total_bytes;                                                                \
    if (!for_kernel_variant((E)->hm.nv, [&](auto nvc_) {                                                     \
          hipLaunchKernelGGL(KERNEL<decltype(nvc_)::value>, g_, b_, lds_, stream, (E)->d_params, args);      \
        }))                                                                                                  \
      FAIL(-19, "no kernel variant for nv=%d", (E)->hm.nv);                                                  \
  } while (0)

static StepArgs base_args(sumo_engine* E) {
  StepArgs a;
  memset(&a, 0, sizeof a);
  a.state = E->d_state; a.counters = E->d_counters; a.seeds = E->d_seeds; a.state_stride = E->state_stride;
  a.stats = E->d_stats; a.obs_stride = E->obs_stride; a.act_stride = E->act_stride; a.N = E->N;
  a.dbg_fault_env = -1;
  a.dbg_qacc = E->dbg_dump;
  return a;
}

extern "C" int sumo_reset(sumo_handle_t E, const uint64_t* seeds_host, const uint8_t* mask_dev, float* obs_dev, void* stream) {
  if (!E) FAIL(-1, "bad handle");
  HIPCHK(hipSetDevice(E->device));
  hipStream_t s = (hipStream_t)stream;
  if (seeds_host) {
    HIPCHK(hipMemcpyAsync(E->d_seeds, seeds_host, (size_t)E->N * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(E->d_counters, 0, (size_t)E->N * 4 * sizeof(int), s));
  }
  StepArgs a = base_args(E);
  a.mask = mask_dev; a.obs = obs_dev;
  SUMO_DISPATCH(sumo_reset_kernel, E, s, a);
  HIPCHK(hipGetLastError());
  if (seeds_host) HIPCHK(hipStreamSynchronize(s));  // seeds_host may be freed by the caller after return
  return 0;
}

extern "C" int sumo_step(sumo_handle_t E, const float* actions_dev, float* obs_dev, double* info_dev, uint8_t* done_dev,
                         double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  if (!E || !actions_dev || !obs_dev || !info_dev || !done_dev || !ep_r_dev || !ep_dr_dev || !ep_l_dev) FAIL(-1, "bad arguments");
  HIPCHK(hipSetDevice(E->device));
  StepArgs a = base_args(E);
  a.actions = actions_dev; a.obs = obs_dev; a.info = info_dev; a.done = done_dev; a.ep_r = ep_r_dev; a.ep_dr = ep_dr_dev;
  a.ep_l = ep_l_dev;
  // Env steps differ in cost (Newton iterations, contacts) by up to ~1.6x and a launch is only N / (6 * 256) rounds deep, so
  // the slowest workgroups of the last round set the launch time.  Workgroups are dispatched in index order: hand the
  // envs out longest-first, using the work each env reported in its previous step (results do not depend on the order).
  a.trace = E->d_trace;
  int nblocks = E->N;
  if (E->sched && E->N <= SCHED_RANK_MAX) {
    // in-kernel ranking (sched_rank): launch t writes its estimates to cost[t & 1]; its first workgroups rank cost[(t-1) & 1]
    // into perm[(t+1) & 1]; it is itself scheduled by perm[t & 1], ranked during launch t-1 from the estimates of launch t-2
    const long long t = E->sched_t++;
    a.cost = E->d_cost + (size_t)(t & 1) * E->N;
    a.perm = t >= 2 ? E->d_perm + (size_t)(t & 1) * E->N : nullptr;
    if (t >= 1) {
      a.rank_cost = E->d_cost + (size_t)((t - 1) & 1) * E->N;
      a.rank_perm = E->d_perm + (size_t)((t + 1) & 1) * E->N;
      a.rank_blocks = (E->N + WAVE - 1) / WAVE;
      nblocks += a.rank_blocks;
    }
  } else if (E->sched) {
    a.cost = E->d_cost; a.perm = E->perm_valid ? E->d_perm : nullptr;
  }
  if (E->cfrc_mode)   // rne_post: the state this step starts from, for the second launch below
    HIPCHK(hipMemcpyAsync(E->d_state_prev, E->d_state, (size_t)E->N * E->state_stride * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (!for_engine_variant(E, [&](auto nvc_, auto slc_) {
        hipLaunchKernelGGL((sumo_step_kernel<decltype(nvc_)::value, decltype(slc_)::value>), dim3(nblocks), dim3(WAVE), (size_t)E->L.total_bytes,
                           (hipStream_t)stream, E->d_params, a);
      }))
    FAIL(-19, "no kernel variant for nv=%d", E->hm.nv);
  HIPCHK(hipGetLastError());
  if (E->cfrc_mode) {
    CfrcArgs q;
    q.prev_state = E->d_state_prev; q.fbuf = E->d_fbuf; q.cfrc_out = E->d_cfrc;
    StepArgs ac = base_args(E);
    ac.actions = actions_dev; ac.obs = obs_dev; ac.done = done_dev;
    dim3 g_(E->N), b_(WAVE);
    size_t lds_ = (size_t)E->L.total_bytes;
    hipStream_t st_ = (hipStream_t)stream;
    if (!for_kernel_variant(E->hm.nv, [&](auto nvc_) {
          hipLaunchKernelGGL(sumo_cfrc_kernel<decltype(nvc_)::value>, g_, b_, lds_, st_, E->d_params, ac, q);
        }))
      FAIL(-19, "no kernel variant for nv=%d", E->hm.nv);
    HIPCHK(hipGetLastError());
  }
  if (E->sched && E->N > SCHED_RANK_MAX) {   // costs stay below 2^16 (see the step kernel's epilogue)
    HIPCHK(rocprim::radix_sort_pairs_desc(E->d_sort_tmp.get(), E->sort_tmp_bytes, E->d_cost.get(), E->d_cost_sorted.get(), E->d_iota.get(),
                                          E->d_perm.get(), (size_t)E->N, 0, 16, (hipStream_t)stream));
    E->perm_valid = true;
  }
  return 0;
}

extern "C" int sumo_set_cfrc_mode(sumo_handle_t E, int mode) {
  if (!E) FAIL(-1, "bad handle");
  if (mode != 0 && mode != 1) FAIL(-2, "cfrc_mode %d: 0 (zero) or 1 (rne_post)", mode);
  HIPCHK(hipSetDevice(E->device));
  if (mode && !E->d_state_prev) {
    HIPCHK(E->d_state_prev.alloc((size_t)E->N * E->state_stride));
    HIPCHK(E->d_fbuf.alloc((size_t)E->N * 5 * E->L.maxcon));
    HIPCHK(E->d_cfrc.alloc((size_t)E->N * 6 * E->hm.nbody));
    HIPCHK(hipMemset(E->d_cfrc, 0, (size_t)E->N * 6 * E->hm.nbody * sizeof(double)));
  }
  E->cfrc_mode = mode;
  return 0;
}
extern "C" int sumo_set_adjust_z(sumo_handle_t E, double adjust_z) {
  if (!E) FAIL(-1, "bad handle");
  if (!(fabs(adjust_z) <= 1e10)) FAIL(-2, "adjust_z must be finite");
  HIPCHK(hipSetDevice(E->device));
  HIPCHK(hipDeviceSynchronize());   // no launch of this engine may be reading the parameter block
  HIPCHK(hipMemcpy((char*)E->d_params.get() + offsetof(Params, adjust_z), &adjust_z, sizeof(double), hipMemcpyHostToDevice));
  E->adjust_z = adjust_z;
  return 0;
}
extern "C" int sumo_get_cfrc_ext(sumo_handle_t E, double* out) {   // HOST float64 [E][nbody][6] of the last step (rne_post mode)
  if (!E || !out) FAIL(-1, "bad arguments");
  if (!E->d_cfrc) FAIL(-2, "cfrc_mode is zero: nothing was computed");
  HIPCHK(hipSetDevice(E->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, E->d_cfrc, (size_t)E->N * 6 * E->hm.nbody * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
extern "C" int sumo_rollout_status(sumo_handle_t E, int64_t* out4) {
  if (!E) FAIL(-1, "bad handle");
  long long o[4] = {0, 0, E->rollout_tickets < 0 ? 0 : E->rollout_tickets, 0};
  if (E->rollout_tickets >= 0) {
    HIPCHK(hipSetDevice(E->device));
    HIPCHK(hipStreamSynchronize(E->rollout_stream));
    int sc[2];
    unsigned long long st[2];
    HIPCHK(hipMemcpy(sc, E->d_rsched, sizeof sc, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(st, E->d_stats + 9, sizeof st, hipMemcpyDeviceToHost));
    // the counters accumulate over launches: an earlier chunk's abort (whose flag the next launch's memset has cleared) still shows
    const bool cut = sc[1] != 0 || st[0] + st[1] != E->acked_faults;
    E->acked_faults = st[0] + st[1];
    o[0] = cut; o[1] = sc[0]; o[3] = (long long)st[1];
    if (out4) for (int i = 0; i < 4; i++) out4[i] = o[i];
    if (cut)
      FAIL(-20, "fused rollout launch was cut short (abort flag set: %llu expired hand-over waits, %llu hand-over tag / checksum mismatches "
                "since creation; %d of %lld tickets were drawn): the rollout buffers hold unwritten rows and the env states are "
                "partly advanced -- reset the envs before continuing", st[0], st[1], sc[0], E->rollout_tickets);
  } else if (out4) for (int i = 0; i < 4; i++) out4[i] = o[i];
  return 0;
}
extern "C" int sumo_static_layout(sumo_handle_t E) { return E ? E->static_layout : -1; }   // 1: this engine runs the static-Layout kernel variants

extern "C" int sumo_get_state(sumo_handle_t E, double* qpos, double* qvel, double* warm, int32_t* counters) {
  if (!E) FAIL(-1, "bad handle");
  HIPCHK(hipSetDevice(E->device));
  HIPCHK(hipDeviceSynchronize());
  const sumo_model_t* m = &E->hm;
  size_t N = (size_t)E->N;
  std::vector<double> st(N * E->state_stride);
  std::vector<int> cn(N * 4);
  HIPCHK(hipMemcpy(st.data(), E->d_state, st.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cn.data(), E->d_counters, cn.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (size_t e = 0; e < N; e++) {
    const double* s = &st[e * E->state_stride];
    if (qpos) memcpy(qpos + e * m->nq, s, m->nq * sizeof(double));
    if (qvel) memcpy(qvel + e * m->nv, s + m->nq, m->nv * sizeof(double));
    if (warm) memcpy(warm + e * m->nv, s + m->nq + m->nv, m->nv * sizeof(double));
    if (counters) { counters[2 * e] = cn[4 * e]; counters[2 * e + 1] = cn[4 * e + 1]; }
  }
  return 0;
}

extern "C" int sumo_set_state(sumo_handle_t E, const double* qpos, const double* qvel, const double* warm, const int32_t* counters) {
  if (!E) FAIL(-1, "bad handle");
  HIPCHK(hipSetDevice(E->device));
  HIPCHK(hipDeviceSynchronize());
  const sumo_model_t* m = &E->hm;
  size_t N = (size_t)E->N;
  std::vector<double> st(N * E->state_stride);
  std::vector<int> cn(N * 4);
  HIPCHK(hipMemcpy(st.data(), E->d_state, st.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cn.data(), E->d_counters, cn.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (size_t e = 0; e < N; e++) {
    double* s = &st[e * E->state_stride];
    if (qpos) memcpy(s, qpos + e * m->nq, m->nq * sizeof(double));
    if (qvel) memcpy(s + m->nq, qvel + e * m->nv, m->nv * sizeof(double));
    if (warm) memcpy(s + m->nq + m->nv, warm + e * m->nv, m->nv * sizeof(double));
    if (counters) { cn[4 * e] = counters[2 * e]; cn[4 * e + 1] = counters[2 * e + 1]; }
  }
  HIPCHK(hipMemcpy(E->d_state, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(E->d_counters, cn.data(), cn.size() * sizeof(int), hipMemcpyHostToDevice));
  return 0;
}

// ---- snapshots (include/sumo_hip.h): host-side copies of the buffers that are state, no kernel
struct SnapshotHeader {
  uint64_t magic;
  uint32_t version;
  int32_t N, state_stride, nq, nv, cfrc_mode;
  uint32_t rollout_seq;      // fused launches so far: the hand-over tags in counters[2] derive from it
  uint32_t pad;
  double adjust_z;
  uint64_t model_hash;       // FNV-1a over the model blob
  uint64_t payload_bytes;
};
static_assert(sizeof(SnapshotHeader) == SUMO_SNAPSHOT_HEADER_BYTES, "snapshot header layout");

static uint64_t blob_hash(const std::vector<char>& b) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (char ch : b) { h ^= (unsigned char)ch; h *= 0x100000001B3ull; }
  return h;
}
// the payload's parts in order: (device pointer, bytes); the cfrc parts only where rne_post has allocated them
struct SnapshotPart { void* dev; size_t bytes; };
static int snapshot_parts(const sumo_engine* E, SnapshotPart* out) {
  const size_t N = (size_t)E->N;
  int n = 0;
  out[n++] = {E->d_state.get(), N * E->state_stride * sizeof(double)};
  out[n++] = {E->d_counters.get(), N * 4 * sizeof(int)};
  out[n++] = {E->d_seeds.get(), N * sizeof(uint64_t)};
  if (E->cfrc_mode && E->d_state_prev) {
    out[n++] = {E->d_state_prev.get(), N * E->state_stride * sizeof(double)};
    out[n++] = {E->d_cfrc.get(), N * 6 * E->hm.nbody * sizeof(double)};
  }
  return n;
}
static size_t snapshot_payload_bytes(const sumo_engine* E) {
  SnapshotPart p[5];
  size_t total = 0;
  for (int i = 0, n = snapshot_parts(E, p); i < n; i++) total += p[i].bytes;
  return total;
}

extern "C" size_t sumo_snapshot_bytes(sumo_handle_t E) { return E ? sizeof(SnapshotHeader) + snapshot_payload_bytes(E) : 0; }

extern "C" int sumo_snapshot_save(sumo_handle_t E, void* dst_host, size_t bytes) {
  if (!E || !dst_host) FAIL(-1, "snapshot: NULL handle or buffer");
  const size_t payload = snapshot_payload_bytes(E);
  if (bytes < sizeof(SnapshotHeader) + payload) FAIL(-30, "snapshot: buffer of %zu bytes, %zu needed (sumo_snapshot_bytes)", bytes, sizeof(SnapshotHeader) + payload);
  HIPCHK(hipSetDevice(E->device));
  HIPCHK(hipDeviceSynchronize());
  SnapshotHeader hd;
  memset(&hd, 0, sizeof hd);
  hd.magic = SUMO_SNAPSHOT_MAGIC; hd.version = SUMO_SNAPSHOT_VERSION;
  hd.N = E->N; hd.state_stride = E->state_stride; hd.nq = E->hm.nq; hd.nv = E->hm.nv; hd.cfrc_mode = E->cfrc_mode;
  hd.rollout_seq = E->rollout_seq; hd.adjust_z = E->adjust_z; hd.model_hash = blob_hash(E->blob); hd.payload_bytes = payload;
  memcpy(dst_host, &hd, sizeof hd);
  char* dst = (char*)dst_host + sizeof hd;
  SnapshotPart p[5];
  for (int i = 0, n = snapshot_parts(E, p); i < n; i++) {
    HIPCHK(hipMemcpy(dst, p[i].dev, p[i].bytes, hipMemcpyDeviceToHost));
    dst += p[i].bytes;
  }
  return 0;
}

extern "C" int sumo_snapshot_load(sumo_handle_t E, const void* src_host, size_t bytes) {
  if (!E || !src_host) FAIL(-1, "snapshot: NULL handle or buffer");
  if (bytes < sizeof(SnapshotHeader)) FAIL(-30, "snapshot: %zu bytes are fewer than a header (%zu)", bytes, sizeof(SnapshotHeader));
  SnapshotHeader hd;
  memcpy(&hd, src_host, sizeof hd);
  if (hd.magic != SUMO_SNAPSHOT_MAGIC) FAIL(-31, "snapshot: bad magic %016llx (not an env snapshot)", (unsigned long long)hd.magic);
  if (hd.version != SUMO_SNAPSHOT_VERSION) FAIL(-32, "snapshot: version %u, this library reads version %d", hd.version, SUMO_SNAPSHOT_VERSION);
  if (hd.N != E->N) FAIL(-33, "snapshot: taken of %d envs, this engine has %d", hd.N, E->N);
  if (hd.state_stride != E->state_stride || hd.nq != E->hm.nq || hd.nv != E->hm.nv)
    FAIL(-34, "snapshot: state rows of another scene (stride %d nq %d nv %d; this engine: stride %d nq %d nv %d)", hd.state_stride, hd.nq, hd.nv,
         E->state_stride, E->hm.nq, E->hm.nv);
  if (hd.model_hash != blob_hash(E->blob)) FAIL(-35, "snapshot: taken with another model (blob hash %016llx, this engine %016llx)",
                                                (unsigned long long)hd.model_hash, (unsigned long long)blob_hash(E->blob));
  if (hd.cfrc_mode != E->cfrc_mode) FAIL(-36, "snapshot: taken in cfrc_mode %d, this engine is in cfrc_mode %d", hd.cfrc_mode, E->cfrc_mode);
  const size_t payload = snapshot_payload_bytes(E);
  if (hd.payload_bytes != payload || bytes < sizeof(SnapshotHeader) + payload)
    FAIL(-37, "snapshot: %zu bytes with a payload of %llu, %zu + %zu needed", bytes, (unsigned long long)hd.payload_bytes, sizeof(SnapshotHeader), payload);
  if (!(fabs(hd.adjust_z) <= 1e10)) FAIL(-38, "snapshot: adjust_z is not finite");
  HIPCHK(hipSetDevice(E->device));
  HIPCHK(hipDeviceSynchronize());   // no launch of this engine may be reading the state or the parameter block
  const char* src = (const char*)src_host + sizeof hd;
  SnapshotPart p[5];
  for (int i = 0, n = snapshot_parts(E, p); i < n; i++) {
    HIPCHK(hipMemcpy(p[i].dev, src, p[i].bytes, hipMemcpyHostToDevice));
    src += p[i].bytes;
  }
  if (hd.adjust_z != E->adjust_z) {
    HIPCHK(hipMemcpy((char*)E->d_params.get() + offsetof(Params, adjust_z), &hd.adjust_z, sizeof(double), hipMemcpyHostToDevice));
    E->adjust_z = hd.adjust_z;
  }
  E->rollout_seq = hd.rollout_seq;
  return 0;
}

extern "C" int sumo_stats(sumo_handle_t E, double* out) {
  if (!E || !out) FAIL(-1, "bad arguments");
  HIPCHK(hipSetDevice(E->device));
  HIPCHK(hipDeviceSynchronize());
  unsigned long long h[SUMO_NSTATS];
  HIPCHK(hipMemcpy(h, E->d_stats, sizeof h, hipMemcpyDeviceToHost));
  for (int i = 0; i < SUMO_NSTATS; i++) out[i] = (double)h[i];
  return 0;
}
