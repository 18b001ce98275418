// engine_host_debug.h -- the development exports: sumo_debug_*, sumo_profile, and WaveOpsArgs with sumo_wave_ops_kernel.  It stays
// the last part, so that kernel remains the last device definition of the unit.  Not in a shard object.
// A part of the sumo_engine.hip translation unit, not a stand-alone header: no includes of its own.

#ifdef SUMO_POLICY_PROBE
extern "C" int sumo_debug_tprobe(double* out8, int reset) {   // development: ticks (100 MHz) inside the five sections of trunk_forward
  unsigned long long h[8];
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_tprobe), sizeof h));
  for (int k = 0; k < 8; k++) out8[k] = (double)h[k];
  if (reset) { memset(h, 0, sizeof h); HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_tprobe), h, sizeof h)); }
  return 0;
}
#endif
// The three host-only exports (no device is touched) run sumo_create's own prepare_scene, up to the stage they report.
// The Layout of a scene, as ints in declaration order; returns the count.  tools/gen_static_layout.py turns it into csrc/layout_static.h.
extern "C" int sumo_debug_layout(const void* model_blob, size_t nbytes, int32_t* out, int cap) {
  if (!model_blob || !out) FAIL(-1, "bad arguments");
  Scene sc;
  if (int rc = prepare_scene(sc, model_blob, nbytes, SCENE_LAYOUT)) return rc;
  const int n = (int)(sizeof(Layout) / sizeof(int));
  if (cap < n) FAIL(-2, "need room for %d ints", n);
  memcpy(out, &sc.L, sizeof(Layout));
  return n;
}
// The two packed role words of the 64 lanes (LaneRec::role0 / role1; the ROLE0_* / ROLE1_* fields), out[2 * lane], out[2 * lane + 1];
// returns the count, or the error sumo_create gives for a scene whose roles do not fit.
extern "C" int sumo_debug_lane_roles(const void* model_blob, size_t nbytes, uint32_t* out, int cap) {
  if (!model_blob || !out) FAIL(-1, "bad arguments");
  Scene sc;
  if (int rc = prepare_scene(sc, model_blob, nbytes, SCENE_ROLES)) return rc;
  if (cap < 2 * WAVE) FAIL(-2, "need room for %d words", 2 * WAVE);
  for (int l = 0; l < WAVE; l++) { out[2 * l] = sc.lanes[l].role0; out[2 * l + 1] = sc.lanes[l].role1; }
  return 2 * WAVE;
}
// The integer members of the compiled model view (model_ints) and of Aux; returns the two counts, the second shifted left by 16.
extern "C" int sumo_debug_model_ints(const void* model_blob, size_t nbytes, int32_t* out, int cap, int32_t* aux_out, int aux_cap) {
  if (!model_blob || !out || !aux_out) FAIL(-1, "bad arguments");
  Scene sc;
  if (int rc = prepare_scene(sc, model_blob, nbytes, SCENE_AUX)) return rc;
  if (cap < 128 || aux_cap < AUX_NINTS) FAIL(-2, "buffers too small");
  const int n = model_ints(&sc.hm, out);
  memcpy(aux_out, &sc.aux.ndepth, AUX_NINTS * sizeof(int));
  return n | (AUX_NINTS << 16);
}
extern "C" int sumo_debug_dump(sumo_handle_t E, double* dev_buf /* [2][8][64] or NULL */) {   // development (-DSUMO_DBG_DUMP builds)
  if (!E) FAIL(-1, "bad handle");
  E->dbg_dump = dev_buf;
  return 0;
}
extern "C" int sumo_debug_fault(sumo_handle_t E, int env) {
  if (!E) FAIL(-1, "bad handle");
  E->dbg_fault_env = env;
  return 0;
}
extern "C" int sumo_debug_trace(sumo_handle_t E, uint64_t* stamps_dev) {
  if (!E) FAIL(-1, "bad handle");
  E->d_trace = (unsigned long long*)stamps_dev;
  return 0;
}

extern "C" int sumo_debug_forward(sumo_handle_t E, const double* ctrl, double* qacc, int32_t* counts) {
  if (!E || !ctrl || !qacc || !counts) FAIL(-1, "bad arguments");
  HIPCHK(hipSetDevice(E->device));
  const sumo_model_t* m = &E->hm;
  size_t N = (size_t)E->N;
  DevBuf<double> d_ctrl, d_qacc;
  DevBuf<int> d_cnt;
  HIPCHK(d_ctrl.alloc(N * m->nu));
  HIPCHK(d_qacc.alloc(N * m->nv));
  HIPCHK(d_cnt.alloc(N * 4));
  HIPCHK(hipMemcpy(d_ctrl, ctrl, N * m->nu * sizeof(double), hipMemcpyHostToDevice));
  StepArgs a = base_args(E);
  a.stats = nullptr; a.dbg_ctrl = d_ctrl; a.dbg_qacc = d_qacc; a.dbg_counts = d_cnt;
  SUMO_DISPATCH(sumo_forward_kernel, E, (hipStream_t)0, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(qacc, d_qacc, N * m->nv * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(counts, d_cnt, N * 4 * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

// One wave through the in-wave primitives of the kernels above, on caller-given lanes (sumo_debug_wave_ops).
struct WaveOpsArgs {
  const double* in;   // [8][64]
  const int* iin;     // [64]
  double* sums;       // [20]: wave_sum of rows 0 .. 7, wave_sum2 of rows 0 .. 1, wave_sum4 of rows 0 .. 3, wave_sum_n<6> of rows 0 .. 5
  double* swapped;    // [64]: pair_swap_f64 of row 0
  int* scan;          // [65]: wave_excl_scan of iin, then its total
  const double* gn;   // [ngn]
  unsigned char* grad;   // [ngn][2]: the gradient test on gn[i], sqrt form and threshold form
  int ngn;
  double scale, tol, thresh;
};
__global__ void __launch_bounds__(WAVE) sumo_wave_ops_kernel(WaveOpsArgs a) {
  const int lane = threadIdx.x;
  double r[8];
  for (int k = 0; k < 8; k++) r[k] = a.in[WAVE * k + lane];
  for (int k = 0; k < 8; k++) { const double s = wave_sum(r[k]); if (lane == 0) a.sums[k] = s; }
  { double p = r[0], q = r[1]; wave_sum2(p, q); if (lane == 0) { a.sums[8] = p; a.sums[9] = q; } }
  { double p = r[0], q = r[1], u = r[2], v = r[3]; wave_sum4(p, q, u, v); if (lane == 0) { a.sums[10] = p; a.sums[11] = q; a.sums[12] = u; a.sums[13] = v; } }
  { double v[6] = {r[0], r[1], r[2], r[3], r[4], r[5]}; wave_sum_n(v); if (lane == 0) for (int k = 0; k < 6; k++) a.sums[14 + k] = v[k]; }
  a.swapped[lane] = pair_swap_f64(r[0]);
  int tot;
  a.scan[lane] = wave_excl_scan(a.iin[lane], lane, &tot);
  if (lane == 0) a.scan[WAVE] = tot;
  for (int i = lane; i < a.ngn; i += WAVE) {
    const double gn = a.gn[i];
    a.grad[2 * i] = a.scale * sqrt(gn) < a.tol;
    a.grad[2 * i + 1] = gn <= a.thresh;
  }
}
extern "C" int sumo_debug_grad_threshold(double scale, double tol, double* out) {   // host only
  if (!out) FAIL(-1, "bad arguments");
  *out = grad_threshold(scale, tol);
  return 0;
}
extern "C" int sumo_debug_wave_ops(sumo_handle_t E, const double* in64x8, const int32_t* int_in64, double* sums20, double* swapped64,
                                   int32_t* scan65, const double* gn, int ngn, double scale, double tol, uint8_t* grad_out) {
  if (!E || !in64x8 || !int_in64 || !sums20 || !swapped64 || !scan65 || ngn < 0 || (ngn && (!gn || !grad_out))) FAIL(-1, "bad arguments");
  HIPCHK(hipSetDevice(E->device));
  DevBuf<double> d_in, d_sums, d_swapped, d_gn;
  DevBuf<int> d_iin, d_scan;
  DevBuf<unsigned char> d_grad;
  const size_t ng = ngn ? (size_t)ngn : 1;
  HIPCHK(d_in.alloc(8 * WAVE)); HIPCHK(d_sums.alloc(20)); HIPCHK(d_swapped.alloc(WAVE)); HIPCHK(d_gn.alloc(ng));
  HIPCHK(d_iin.alloc(WAVE)); HIPCHK(d_scan.alloc(WAVE + 1)); HIPCHK(d_grad.alloc(2 * ng));
  HIPCHK(hipMemcpy(d_in, in64x8, 8 * WAVE * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_iin, int_in64, WAVE * sizeof(int), hipMemcpyHostToDevice));
  if (ngn) HIPCHK(hipMemcpy(d_gn, gn, ng * sizeof(double), hipMemcpyHostToDevice));
  WaveOpsArgs a{d_in, d_iin, d_sums, d_swapped, d_scan, d_gn, d_grad, ngn, scale, tol, grad_threshold(scale, tol)};
  hipLaunchKernelGGL(sumo_wave_ops_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)0, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(sums20, d_sums, 20 * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(swapped64, d_swapped, WAVE * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(scan65, d_scan, (WAVE + 1) * sizeof(int), hipMemcpyDeviceToHost));
  if (ngn) HIPCHK(hipMemcpy(grad_out, d_grad, 2 * ng * sizeof(unsigned char), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int sumo_profile(sumo_handle_t E, double* out24) {  // cycle totals per phase (SUMO_PROFILE builds only)
  if (!E || !out24) FAIL(-1, "bad arguments");
  HIPCHK(hipSetDevice(E->device));
  HIPCHK(hipDeviceSynchronize());
  unsigned long long h[48];
  HIPCHK(hipMemcpy(h, E->d_stats, sizeof h, hipMemcpyDeviceToHost));
  for (int i = 0; i < 24; i++) out24[i] = (double)h[16 + i];
  return 0;
}
