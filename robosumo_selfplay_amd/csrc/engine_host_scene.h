// engine_host_scene.h -- the reset / forward kernels and the host's scene preparation: SUMO_FOR_NV, FAIL / HIPCHK, Scene,
// SceneOptions, DevBuf, sumo_engine, build_aux .. prepare_scene.  Not in a shard object.
// A part of the sumo_engine.hip translation unit, not a stand-alone header: no includes of its own.

template <int NV>
__global__ void __launch_bounds__(WAVE) sumo_reset_kernel(const Params* P, StepArgs a) {
  Ctx<NV> c;
  ctx_init(c, P, smem_dyn);
  const sumo_model_t& mdl = P->mdl;
  const int e = blockIdx.x, lane = c.lane;
  if (e >= a.N) return;
  if (a.mask && !a.mask[e]) return;
  int* cnt = a.counters + 4 * e;
  int reset_count = cnt[1];
  reset_state(c, a.seeds[e], (uint32_t)reset_count);
  if (a.obs) write_obs(c, a.obs + (size_t)e * 2 * a.obs_stride, a.obs_stride, 0);
  store_state(c, a, e);
  if (lane == 0) {
    double* st = a.state + (size_t)e * a.state_stride;
    cnt[0] = 0; cnt[1] = reset_count + 1;
    st[mdl.nq + 2 * mdl.nv] = 0; st[mdl.nq + 2 * mdl.nv + 1] = 0;
  }
}

template <int NV>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(SUMO_WPE_OF(NV), SUMO_WPE_OF(NV)))) sumo_forward_kernel(const Params* P, StepArgs a) {
  Ctx<NV> c;
  ctx_init(c, P, smem_dyn);
  const sumo_model_t& mdl = P->mdl;
  const int e = blockIdx.x, lane = c.lane;
  if (e >= a.N) return;
  load_state(c, a, e);
  if (lane < mdl.nu) S(ctrl)[lane] = a.dbg_ctrl[(size_t)e * mdl.nu + lane];
  SYNC();
  forward(c);
  if (lane < mdl.nv) a.dbg_qacc[(size_t)e * mdl.nv + lane] = S(x)[lane];
  if (lane == 0) {
    int* o = a.dbg_counts + 4 * e;
    o[0] = c.ncon; o[1] = c.nefc; o[2] = c.st_newton; o[3] = c.ndropped;
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
#ifdef SUMO_DEV_NV  /* development builds: compile a single kernel variant */
#define SUMO_FOR_NV(X) X(SUMO_DEV_NV)
#else
#define SUMO_FOR_NV(X) X(28) X(32) X(36) X(40) X(44)
#endif
static thread_local char g_err[512];
extern "C" const char* sumo_last_error(void) { return g_err; }
#define FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return code; } while (0)
#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) FAIL(-100, "%s failed: %s", #expr, hipGetErrorString(_e)); } while (0)

// Everything the host derives from a model blob, with one owner.  prepare_scene fills it stage by stage; it makes no HIP call (the
// host-only exports run where there is no device), and it is not copyable: hm points into blob.
struct Scene {
  Scene() = default;
  Scene(const Scene&) = delete;
  Scene& operator=(const Scene&) = delete;
  std::vector<char> blob;
  sumo_model_t hm{};                       // host view of blob
  Aux aux{};                               // its table pointers stay null here: sumo_create points the device copy at the uploads
  Layout L{};
  std::vector<int> ai;                     // the tables behind aux.ai / aux.af / aux.pic
  std::vector<double> af;
  std::vector<signed char> pic;
  std::vector<LaneRec> lanes;
  std::vector<int> pair_rec;
  std::vector<float> pair_bound;
  double grad_thresh = -1.0;               // Params::grad_thresh
  int static_layout = 0;                   // 1 / 2: the scene's Layout equals a compile-time table (Ant-vs-Ant / Spider-vs-Spider): static kernel variants
  int state_stride = 0, obs_stride = 0, act_stride = 0;
};

// What the environment says about a scene preparation, read once per preparation.
struct SceneOptions {
  bool true_tree;      // SUMO_TRUE_TREE != 0: the model's own body tree instead of the effective one
  int maxcon;          // SUMO_MAXCON > 0: contact records (still capped by what the line search holds in registers)
  int warm_mode;       // SUMO_WARM_MODE (Layout::warm_mode)
  int force_dense;     // SUMO_FORCE_DENSE_H (Layout::force_dense)
  bool no_tree;        // SUMO_NO_TREE != 0: never the tree solver
  bool jbcap_set;      // SUMO_JBCAP present, whatever its value: the Jacobian pool does not grow into the spare LDS
  int jbcap;           // SUMO_JBCAP > 0: the pool's capacity
  bool static_layout;  // unless SUMO_STATIC_LAYOUT is 0: the static kernel variants where the scene matches a compile-time table
  static SceneOptions from_env() {
    auto num = [](const char* name) { const char* v = getenv(name); return v ? atoi(v) : 0; };
    const char* sl = getenv("SUMO_STATIC_LAYOUT");
    return {num("SUMO_TRUE_TREE") != 0, num("SUMO_MAXCON"), num("SUMO_WARM_MODE"), num("SUMO_FORCE_DENSE_H"), num("SUMO_NO_TREE") != 0,
            getenv("SUMO_JBCAP") != nullptr, num("SUMO_JBCAP"), !(sl && atoi(sl) == 0)};
  }
};

// Device memory that is freed with its holder.  Reads like the raw pointer it replaces; templates that deduce a pointer type take get().
template <class T>
struct DevBuf {
  struct Free { void operator()(T* p) const { (void)hipFree(p); } };
  std::unique_ptr<T, Free> p;
  T* get() const { return p.get(); }
  operator T*() const { return p.get(); }
  hipError_t alloc(size_t n) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, n * sizeof(T));
    if (e == hipSuccess) p.reset((T*)q);
    return e;
  }
  hipError_t upload(const std::vector<T>& h) {
    const hipError_t e = alloc(h.size());
    return e != hipSuccess ? e : hipMemcpy(p.get(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
  }
};

struct sumo_engine : Scene {   // a prepared scene and the device state of its N envs
  int device = 0, N = 0;
  DevBuf<Params> d_params;
  DevBuf<LaneRec> d_lanes;
  DevBuf<int> d_pair_rec;
  DevBuf<float> d_pair_bound;
  DevBuf<char> d_blob;
  DevBuf<int> d_ai;
  DevBuf<double> d_af;
  DevBuf<signed char> d_pic;
  DevBuf<double> d_state;
  int cfrc_mode = 0;                       // 0 zero (reference behaviour), 1 rne_post (sumo_set_cfrc_mode)
  double adjust_z = 0.0;                   // Agent._adjust_z (sumo_set_adjust_z)
  DevBuf<double> d_state_prev, d_fbuf, d_cfrc;   // rne_post: pre-step state, row-force scratch, cfrc_ext [N][nbody][6] (sumo_set_cfrc_mode allocates them)
  DevBuf<int> d_counters;
  DevBuf<uint64_t> d_seeds;
  DevBuf<unsigned long long> d_stats;
  // longest-first scheduling of the env steps (see sumo_step)
  DevBuf<int> d_cost, d_cost_sorted, d_iota, d_perm;   // d_cost / d_perm: two buffers of N each
  unsigned long long* d_trace = nullptr;   // sumo_debug_trace: the caller's buffer, not owned
  int num_cus = 0;                         // cached device property (sumo_rollout_steps sizes its persistent grid with it)
  DevBuf<int> d_rsched;                    // sumo_rollout_steps: ticket counter, abort flag, per-env progress [2 + N] (allocated by the first fused launch)
  unsigned rollout_seq = 0;                // fused launches so far (hand-over tags: seq_base = (rollout_seq & 0x7FFF) << 16)
  hipStream_t rollout_stream = nullptr;    // stream of the most recent fused launch (sumo_rollout_status waits on it)
  long long rollout_tickets = -1;          // N * K of the most recent fused launch, -1: none yet
  int dbg_fault_env = -1;                  // sumo_debug_fault
  double* dbg_dump = nullptr;              // sumo_debug_dump (SUMO_DBG_DUMP builds): the caller's buffer, not owned
  unsigned long long acked_faults = 0;     // stats[9] + stats[10] already reported by sumo_rollout_status
  long long sched_t = 0;                                                                     // step launches so far (in-kernel ranking)
  DevBuf<char> d_sort_tmp;
  size_t sort_tmp_bytes = 0;
  bool sched = true, perm_valid = false;
};

static void quat2mat_h(double* m, const double* q) {
  double w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}

// build_aux: the derived tables (S.ai / af / pic, the Aux offsets into them), the lane records and the pair records of a parsed
// scene.  Its pieces run in the order they are declared in; the members are what one piece leaves for the later ones.
namespace {
struct AuxBuilder {
  Scene& S;
  const SceneOptions& opt;
  const sumo_model_t* const m = &S.hm;
  const int nb = m->nbody, nv = m->nv;
  Aux& A = S.aux;
  std::vector<int>& ai = S.ai;
  std::vector<double>& af = S.af;
  std::vector<signed char>& pic = S.pic;
  const int* const tparent = SUMO_I(m, body_parentid);
  const int* const gbody = SUMO_I(m, geom_bodyid);
  const int* const gtype = SUMO_I(m, geom_type);
  const int* parent = nullptr;   // tparent, or eparent: the tree the kernels walk
  bool folded = false;           // parent is the effective tree
  std::vector<int> eparent, depth, lvl_adr, lvl_body, is_stub, child_adr, child;
  std::vector<double> epos, equat;
  std::vector<int> chain_len, chain, bchain_len, bchain, body_agent, tri_i, tri_j, cen_of_geom;
  int push_tbl(const std::vector<int>& v) { int o = (int)ai.size(); ai.insert(ai.end(), v.begin(), v.end()); return o; }
  void effective_tree();
  int chains_and_checks();
  int collision_tables();
  int lane_records();
  void hessian_entries();
  int pair_records();
};
}  // namespace

static int build_aux(Scene& S, const SceneOptions& opt) {
  const sumo_model_t* m = &S.hm;
  int nb = m->nbody, nv = m->nv;
  if (nb > WAVE || nv > WAVE || m->njnt > WAVE || m->nq > WAVE) FAIL(-10, "scene too large for one wavefront per env (nbody %d nv %d)", nb, nv);
  if (m->nagent != 2) FAIL(-11, "exactly two agents expected");
  if (nv != 28 && nv != 32 && nv != 36 && nv != 40 && nv != 44) FAIL(-18, "no kernel variant for nv=%d", nv);
  AuxBuilder B{S, opt};
  B.effective_tree();
  if (int rc = B.chains_and_checks()) return rc;
  if (int rc = B.collision_tables()) return rc;
  if (int rc = B.lane_records()) return rc;
  B.hessian_entries();
  return B.pair_records();
}

void AuxBuilder::effective_tree() {
  // "Effective" tree of the kernel's level-by-level passes: a body whose parent carries no joint is re-attached to the nearest
  // ancestor that does, with the static transforms composed (the jointless body keeps its own frame as a leaf: its frame
  // still feeds its geom and inertia, and subtree sums do not care which rigidly connected ancestor collects it).  For the
  // RoboSumo agents (torso -> jointless leg stub -> hip body -> ankle body) this removes one level from every pass.
  eparent.assign(nb, 0);
  epos.assign(3 * (size_t)nb, 0.0); equat.assign(4 * (size_t)nb, 0.0);
  for (int b = 0; b < nb; b++) {
    double pos[3] = {SUMO_F(m, body_pos)[3 * b], SUMO_F(m, body_pos)[3 * b + 1], SUMO_F(m, body_pos)[3 * b + 2]};
    double q[4] = {SUMO_F(m, body_quat)[4 * b], SUMO_F(m, body_quat)[4 * b + 1], SUMO_F(m, body_quat)[4 * b + 2], SUMO_F(m, body_quat)[4 * b + 3]};
    int pp = b ? tparent[b] : 0;
    while (pp != 0 && SUMO_I(m, body_jntnum)[pp] == 0) {
      const double* pq = SUMO_F(m, body_quat) + 4 * pp;
      const double* ppos = SUMO_F(m, body_pos) + 3 * pp;
      double R[9];
      quat2mat_h(R, pq);
      double np_[3] = {ppos[0] + R[0] * pos[0] + R[1] * pos[1] + R[2] * pos[2], ppos[1] + R[3] * pos[0] + R[4] * pos[1] + R[5] * pos[2],
                       ppos[2] + R[6] * pos[0] + R[7] * pos[1] + R[8] * pos[2]};
      double nq[4] = {pq[0] * q[0] - pq[1] * q[1] - pq[2] * q[2] - pq[3] * q[3], pq[0] * q[1] + pq[1] * q[0] + pq[2] * q[3] - pq[3] * q[2],
                      pq[0] * q[2] - pq[1] * q[3] + pq[2] * q[0] + pq[3] * q[1], pq[0] * q[3] + pq[1] * q[2] - pq[2] * q[1] + pq[3] * q[0]};
      double nn = sqrt(nq[0] * nq[0] + nq[1] * nq[1] + nq[2] * nq[2] + nq[3] * nq[3]);
      for (int k = 0; k < 3; k++) pos[k] = np_[k];
      for (int k = 0; k < 4; k++) q[k] = nq[k] / nn;
      pp = tparent[pp];
    }
    eparent[b] = pp;
    for (int k = 0; k < 3; k++) epos[3 * b + k] = pos[k];
    for (int k = 0; k < 4; k++) equat[4 * b + k] = q[k];
  }
  parent = opt.true_tree ? tparent : eparent.data();
  folded = parent != tparent;
  depth.assign(nb, 0);
  int ndepth = 1;
  for (int b = 1; b < nb; b++) { depth[b] = depth[parent[b]] + 1; if (depth[b] + 1 > ndepth) ndepth = depth[b] + 1; }
  A.ndepth = ndepth;
  lvl_adr.assign(ndepth + 1, 0);
  for (int d = 0; d < ndepth; d++) { lvl_adr[d] = (int)lvl_body.size(); for (int b = 0; b < nb; b++) if (depth[b] == d) lvl_body.push_back(b); }
  lvl_adr[ndepth] = (int)lvl_body.size();
  // jointless leaves of the effective tree ("stubs", e.g. the fixed upper leg segments): rigidly attached to their parent, so
  // their inertia is added to the parent's once per evaluation and they take no part in the subtree gathers
  is_stub.assign(nb, 0);
  if (folded)
    for (int b = 1; b < nb; b++) {
      if (SUMO_I(m, body_jntnum)[b] != 0 || parent[b] == 0) continue;
      bool leaf = true;
      for (int ch = 1; ch < nb; ch++) if (ch != b && parent[ch] == b) leaf = false;
      is_stub[b] = leaf;
    }
  child_adr.assign(nb + 1, 0);
  for (int b = 0; b < nb; b++) {
    child_adr[b] = (int)child.size();
    for (int ch = nb - 1; ch > b; ch--) if (parent[ch] == b && b != 0 && !is_stub[ch]) child.push_back(ch);
  }
  child_adr[nb] = (int)child.size();
}

// dof and body chains root -> body, the checks of what the kernels assume about a body, and the integer tables
int AuxBuilder::chains_and_checks() {
  chain_len.assign(nb, 0); chain.assign(nb * MAXCHAIN, -1); bchain_len.assign(nb, 0); bchain.assign(nb * MAXBCHAIN, -1); body_agent.assign(nb, -1);
  pic.assign((size_t)nb * nv, -1);
  const int* dofnum = SUMO_I(m, body_dofnum);
  const int* dofadr = SUMO_I(m, body_dofadr);
  const int* dpar = SUMO_I(m, dof_parentid);
  for (int b = 1; b < nb; b++) {
    std::vector<int> bc;
    for (int k = b; k != 0; k = parent[k]) bc.insert(bc.begin(), k);
    if ((int)bc.size() > MAXBCHAIN) FAIL(-12, "kinematic tree deeper than %d bodies", MAXBCHAIN);
    bchain_len[b] = (int)bc.size();
    for (size_t i = 0; i < bc.size(); i++) bchain[b * MAXBCHAIN + i] = bc[i];
    int bb = b;
    while (bb && dofnum[bb] == 0) bb = tparent[bb];
    std::vector<int> dc;
    if (bb) for (int d = dofadr[bb] + dofnum[bb] - 1; d >= 0; d = dpar[d]) dc.insert(dc.begin(), d);
    if ((int)dc.size() > MAXCHAIN) FAIL(-13, "dof chain longer than %d", MAXCHAIN);
    chain_len[b] = (int)dc.size();
    for (size_t i = 0; i < dc.size(); i++) { chain[b * MAXCHAIN + i] = dc[i]; pic[(size_t)b * nv + dc[i]] = (signed char)i; }
    for (int a = 0; a < m->nagent; a++) {
      int adr = SUMO_I(m, agent_bodyadr)[a];
      if (b >= adr && b < adr + SUMO_I(m, agent_nbody)[a]) body_agent[b] = a;
    }
    if (body_agent[b] < 0) FAIL(-14, "body %d belongs to no agent", b);
    // one geom per moving body, and its frame is the inertial frame (what the kernel assumes)
    int g0 = SUMO_I(m, body_geomadr)[b], g1 = SUMO_I(m, body_geomadr)[b + 1];
    if (g1 - g0 != 1) FAIL(-15, "body %d has %d geoms; the engine needs exactly one per moving body", b, g1 - g0);
    for (int k = 0; k < 3; k++) if (SUMO_F(m, geom_pos)[3 * g0 + k] != SUMO_F(m, body_ipos)[3 * b + k]) FAIL(-16, "geom/inertial frame mismatch");
    for (int k = 0; k < 4; k++) if (SUMO_F(m, geom_quat)[4 * g0 + k] != SUMO_F(m, body_iquat)[4 * b + k]) FAIL(-16, "geom/inertial frame mismatch");
  }
  // one actuator per dof at most (kernel adds actuator forces without atomics)
  {
    std::vector<int> seen(nv, 0);
    for (int u = 0; u < m->nu; u++) { int d = SUMO_I(m, actuator_dofid)[u]; if (seen[d]++) FAIL(-17, "two actuators on one dof"); }
  }
  for (int i = 0; i < nv; i++) for (int j = 0; j <= i; j++) { tri_i.push_back(i); tri_j.push_back(j); }
  A.ntri = (int)tri_i.size();
  A.o_lvl_adr = push_tbl(lvl_adr); A.o_lvl_body = push_tbl(lvl_body); A.o_child_adr = push_tbl(child_adr);
  A.o_child = push_tbl(child.empty() ? std::vector<int>(1, 0) : child);
  A.o_chain_len = push_tbl(chain_len); A.o_chain = push_tbl(chain); A.o_bchain_len = push_tbl(bchain_len);
  A.o_bchain = push_tbl(bchain); A.o_body_agent = push_tbl(body_agent); A.o_tri_i = push_tbl(tri_i); A.o_tri_j = push_tbl(tri_j);
  A.o_wgmat = 0;
  af.assign((size_t)9 * m->ngeom, 0.0);
  for (int g = 0; g < m->ngeom; g++) quat2mat_h(&af[9 * g], SUMO_F(m, geom_quat) + 4 * g);
  return 0;
}

// collision centres (body ids for agent geoms, nbody + w for world geom w) and the static tables the collision code reads by centre
int AuxBuilder::collision_tables() {
  int nworld = SUMO_I(m, body_geomadr)[1] - SUMO_I(m, body_geomadr)[0];
  int nc = nb + nworld;
  if (nc > 255) FAIL(-20, "too many collision centres");
  A.nc = nc; A.nworld = nworld;
  cen_of_geom.assign(m->ngeom, 0);
  std::vector<int> geom_of_cen(nc, -1);
  for (int g = 0; g < m->ngeom; g++) {
    int ci = gbody[g] == 0 ? nb + (g - SUMO_I(m, body_geomadr)[0]) : gbody[g];
    cen_of_geom[g] = ci; geom_of_cen[ci] = g;
  }
  // static double tables: csize[2*nc] | cinvw[nc] | wbox[12*nworld] | wlim[6*nworld]
  A.o_stat_d = (int)af.size();
  {
    std::vector<double> sd((size_t)3 * nc + 18 * nworld, 0.0), wpa((size_t)6 * nworld, 0.0);
    for (int ci = 0; ci < nc; ci++) {
      int g = geom_of_cen[ci];
      if (g >= 0) { sd[2 * ci] = SUMO_F(m, geom_size)[3 * g]; sd[2 * ci + 1] = SUMO_F(m, geom_size)[3 * g + 1]; }
      int body = ci < nb ? ci : 0;
      sd[2 * nc + ci] = SUMO_F(m, body_invweight0)[2 * body];
    }
    const double BIG = 1e300;
    for (int w = 0; w < nworld; w++) {
      int g = SUMO_I(m, body_geomadr)[0] + w;
      double R[9];
      quat2mat_h(R, SUMO_F(m, geom_quat) + 4 * g);
      double* wb = &sd[3 * nc + 12 * w];
      for (int k = 0; k < 9; k++) wb[k] = R[k];
      for (int k = 0; k < 3; k++) wb[9 + k] = SUMO_F(m, geom_size)[3 * g + k];
      // broad-phase extent of the geom in its own frame, hi[3] | lo[3] (the other geom's bounding radius goes into the
      // pair bound): box = its half sizes; capsule / border rod = its axis segment; plane = the half space z <= 0;
      // anything else = its centre with the bounding radius
      double* wl = &sd[3 * nc + 12 * nworld + 6 * w];
      const double* gs = SUMO_F(m, geom_size) + 3 * g;
      if (gtype[g] == SUMO_GEOM_BOX) { for (int k = 0; k < 3; k++) { wl[k] = gs[k]; wl[3 + k] = -gs[k]; } }
      else if (gtype[g] == SUMO_GEOM_CAPSULE || gtype[g] == SUMO_GEOM_CYLINDER) { wl[2] = gs[1]; wl[5] = -gs[1]; }
      else if (gtype[g] == SUMO_GEOM_PLANE) { wl[0] = wl[1] = BIG; wl[2] = 0; wl[3] = wl[4] = wl[5] = -BIG; }
      for (int k = 0; k < 3; k++) wpa[3 * w + k] = SUMO_F(m, geom_pos)[3 * g + k];
      wpa[3 * nworld + 3 * w + 0] = R[2]; wpa[3 * nworld + 3 * w + 1] = R[5]; wpa[3 * nworld + 3 * w + 2] = R[8];
    }
    A.n_stat_d = (int)sd.size();
    af.insert(af.end(), sd.begin(), sd.end());
    A.o_wpa = (int)af.size();   // world geom positions / axes: read once per launch, not kept in LDS
    af.insert(af.end(), wpa.begin(), wpa.end());
  }
  // static int tables: ctype[nc] | cbody[nc] | chain words [2*nb] | chlen_agent[nb]
  {
    std::vector<int> si((size_t)2 * nc + 3 * nb, 0);
    for (int ci = 0; ci < nc; ci++) {
      int g = geom_of_cen[ci];
      int t = g >= 0 ? gtype[g] : -1;
      if (t == SUMO_GEOM_CYLINDER) t = SUMO_GEOM_CAPSULE;  // border rods collide as capsules
      si[ci] = t; si[nc + ci] = ci < nb ? ci : 0;
    }
    for (int b = 0; b < nb; b++) {
      unsigned w0 = 0, w1 = 0;
      for (int p = 0; p < chain_len[b]; p++) {
        unsigned d = (unsigned)chain[b * MAXCHAIN + p];
        if (p < 4) w0 |= d << (8 * p); else w1 |= d << (8 * (p - 4));
      }
      si[2 * nc + 2 * b] = (int)w0; si[2 * nc + 2 * b + 1] = (int)w1;
      si[2 * nc + 2 * nb + b] = chain_len[b] | ((body_agent[b] < 0 ? 0 : body_agent[b]) << 8);
    }
    A.o_stat_i = push_tbl(si);
    A.n_stat_i = (int)si.size();
  }
  return 0;
}

// per-lane constants: lane l is body l, dof l, joint l and actuator l at once
int AuxBuilder::lane_records() {
  S.lanes.assign(WAVE, LaneRec());
  const int* jbody = SUMO_I(m, jnt_bodyid);
  for (int l = 0; l < WAVE; l++) {
    LaneRec& K = S.lanes[l];
    memset(&K, 0, sizeof K);
    K.b_jnt = -1; K.b_level = -1; K.b_agent = 0;
    if (l < nb) {
      int b = l;
      for (int k = 0; k < 3; k++) { K.b_pos[k] = folded ? epos[3 * b + k] : SUMO_F(m, body_pos)[3 * b + k]; K.b_ipos[k] = SUMO_F(m, body_ipos)[3 * b + k]; K.b_inertia[k] = SUMO_F(m, body_inertia)[3 * b + k]; }
      for (int k = 0; k < 4; k++) { K.b_quat[k] = folded ? equat[4 * b + k] : SUMO_F(m, body_quat)[4 * b + k]; K.b_iquat[k] = SUMO_F(m, body_iquat)[4 * b + k]; }
      K.b_mass = SUMO_F(m, body_mass)[b];
      K.b_parent = parent[b]; K.b_level = depth[b]; K.b_agent = body_agent[b] < 0 ? 0 : body_agent[b];
      int jn = SUMO_I(m, body_jntnum)[b], ja = SUMO_I(m, body_jntadr)[b];
      if (jn > 1) FAIL(-21, "body %d has %d joints; the engine supports at most one per body", b, jn);
      if (jn == 1) {
        K.b_jnt = ja;
        K.b_isfree = SUMO_I(m, jnt_type)[ja] == SUMO_JNT_FREE;
        K.b_qadr = SUMO_I(m, jnt_qposadr)[ja];
        for (int k = 0; k < 3; k++) { K.j_pos[k] = SUMO_F(m, jnt_pos)[3 * ja + k]; K.j_axis[k] = SUMO_F(m, jnt_axis)[3 * ja + k]; }
        K.j_qpos0 = SUMO_F(m, qpos0)[K.b_qadr];
      }
      int c0 = child_adr[b], c1 = child_adr[b + 1];
      K.b_nchild = c1 - c0;
      if (K.b_nchild > 8) FAIL(-22, "body %d has more than 8 children", b);
      if (b > 0 && K.b_nchild > A.maxchild) A.maxchild = K.b_nchild;
      {  // inertial constants for cinert: own, merged with the rigidly attached leaves, or zero for such a leaf
        auto add_part = [&](double* I6, double* mc, double& M, double mass, const double* cpos, const double* Rb, const double* diag) {
          // accumulates mass, mass * centre and the inertia about the ORIGIN of the body frame (shifted to the centre below)
          double Ip[9];
          for (int r = 0; r < 3; r++) for (int cc = 0; cc < 3; cc++)
            Ip[3 * r + cc] = Rb[3 * r] * diag[0] * Rb[3 * cc] + Rb[3 * r + 1] * diag[1] * Rb[3 * cc + 1] + Rb[3 * r + 2] * diag[2] * Rb[3 * cc + 2];
          double d2 = cpos[0] * cpos[0] + cpos[1] * cpos[1] + cpos[2] * cpos[2];
          I6[0] += Ip[0] + mass * (d2 - cpos[0] * cpos[0]); I6[1] += Ip[4] + mass * (d2 - cpos[1] * cpos[1]); I6[2] += Ip[8] + mass * (d2 - cpos[2] * cpos[2]);
          I6[3] += Ip[1] - mass * cpos[0] * cpos[1]; I6[4] += Ip[2] - mass * cpos[0] * cpos[2]; I6[5] += Ip[5] - mass * cpos[1] * cpos[2];
          for (int k = 0; k < 3; k++) mc[k] += mass * cpos[k];
          M += mass;
        };
        double I6[6] = {0, 0, 0, 0, 0, 0}, mc[3] = {0, 0, 0}, M = 0, Rb[9];
        if (!is_stub[b]) {
          quat2mat_h(Rb, SUMO_F(m, body_iquat) + 4 * b);
          add_part(I6, mc, M, SUMO_F(m, body_mass)[b], SUMO_F(m, body_ipos) + 3 * b, Rb, SUMO_F(m, body_inertia) + 3 * b);
          for (int sb = 1; sb < nb; sb++)
            if (is_stub[sb] && parent[sb] == b) {
              double Rs[9], Ri[9], Rsi[9], cs[3];
              quat2mat_h(Rs, &equat[4 * sb]);
              quat2mat_h(Ri, SUMO_F(m, body_iquat) + 4 * sb);
              for (int r = 0; r < 3; r++) for (int cc = 0; cc < 3; cc++)
                Rsi[3 * r + cc] = Rs[3 * r] * Ri[cc] + Rs[3 * r + 1] * Ri[3 + cc] + Rs[3 * r + 2] * Ri[6 + cc];
              const double* ip = SUMO_F(m, body_ipos) + 3 * sb;
              for (int k = 0; k < 3; k++) cs[k] = epos[3 * sb + k] + Rs[3 * k] * ip[0] + Rs[3 * k + 1] * ip[1] + Rs[3 * k + 2] * ip[2];
              add_part(I6, mc, M, SUMO_F(m, body_mass)[sb], cs, Rsi, SUMO_F(m, body_inertia) + 3 * sb);
              A.nstub++;
            }
          double cm[3] = {0, 0, 0};
          if (M > 0) for (int k = 0; k < 3; k++) cm[k] = mc[k] / M;
          // shift from the frame origin to the (merged) centre of mass
          double d2 = cm[0] * cm[0] + cm[1] * cm[1] + cm[2] * cm[2];
          I6[0] -= M * (d2 - cm[0] * cm[0]); I6[1] -= M * (d2 - cm[1] * cm[1]); I6[2] -= M * (d2 - cm[2] * cm[2]);
          I6[3] += M * cm[0] * cm[1]; I6[4] += M * cm[0] * cm[2]; I6[5] += M * cm[1] * cm[2];
          for (int k = 0; k < 6; k++) K.c_I[k] = I6[k];
          for (int k = 0; k < 3; k++) K.c_ipos[k] = cm[k];
          K.c_mass = M;
        }
      }
      for (int q = 0; q < K.b_nchild; q++) K.b_child |= (unsigned long long)child[c0 + q] << (8 * q);
      K.b_bchain_len = bchain_len[b];
      for (int q = 0; q < bchain_len[b]; q++) K.b_bchain |= (unsigned)bchain[b * MAXBCHAIN + q] << (8 * q);
      K.b_chain_len = chain_len[b];
      for (int q = 0; q < chain_len[b]; q++) {
        int d = chain[b * MAXCHAIN + q];
        K.b_chain |= (unsigned long long)d << (8 * q);
        if (SUMO_I(m, dof_bodyid)[d] == b) K.b_chain_own |= 1u << q;
        int jt = SUMO_I(m, dof_jntid)[d];
        if (SUMO_I(m, jnt_type)[jt] == SUMO_JNT_FREE && SUMO_I(m, jnt_dofadr)[jt] == d) K.b_chain_free |= 1u << q;
      }
    }
    if (l < nv) {
      int d = l, b = SUMO_I(m, dof_bodyid)[d];
      K.d_arm = SUMO_F(m, dof_armature)[d]; K.d_damp = SUMO_F(m, dof_damping)[d]; K.d_body = b;
      K.d_pos = pic[(size_t)b * nv + d];
      K.d_hid = -1;
      { int jt = SUMO_I(m, dof_jntid)[d];
        if (SUMO_I(m, jnt_type)[jt] == SUMO_JNT_HINGE) { int h = 0; for (int jj = 0; jj < jt; jj++) if (SUMO_I(m, jnt_type)[jj] == SUMO_JNT_HINGE) h++; K.d_hid = h; } }
      for (int q = 0; q < chain_len[b]; q++) K.d_chain |= (unsigned long long)chain[b * MAXCHAIN + q] << (8 * q);
    }
    if (l < m->njnt) {
      int j = l;
      K.jt_type = SUMO_I(m, jnt_type)[j]; K.jt_qadr = SUMO_I(m, jnt_qposadr)[j]; K.jt_dadr = SUMO_I(m, jnt_dofadr)[j];
      K.jt_limited = SUMO_I(m, jnt_limited)[j]; K.jt_body = jbody[j]; K.jt_agent = body_agent[jbody[j]] < 0 ? 0 : body_agent[jbody[j]];
      K.jt_lo = SUMO_F(m, jnt_range)[2 * j]; K.jt_hi = SUMO_F(m, jnt_range)[2 * j + 1]; K.jt_margin = SUMO_F(m, jnt_margin)[j];
      K.jt_invw = SUMO_F(m, dof_invweight0)[K.jt_dadr];
      K.jt_hid = -1;
      if (K.jt_type == SUMO_JNT_HINGE) { int h = 0; for (int jj = 0; jj < j; jj++) if (SUMO_I(m, jnt_type)[jj] == SUMO_JNT_HINGE) h++; K.jt_hid = h; }
    }
    if (l < m->nu) {
      K.a_dof = SUMO_I(m, actuator_dofid)[l]; K.a_gear = SUMO_F(m, actuator_gear)[l];
      K.a_lo = SUMO_F(m, actuator_ctrlrange)[2 * l]; K.a_hi = SUMO_F(m, actuator_ctrlrange)[2 * l + 1];
    }
  }
  return 0;
}

// lower-triangle entry words of the dense Hessian assembly, entry t = lane + 64 m: (i << 8 | j) | chain position of dof i
// << 16 | of dof j << 20; 0xFFFF = none.  Read where the (rare) dense path assembles H instead of living in 7 registers of
// every lane for the whole launch.
void AuxBuilder::hessian_entries() {
  const int epl = (A.ntri + WAVE - 1) / WAVE;
  std::vector<int> ent((size_t)epl * WAVE, 0xFFFF);
  for (int t = 0; t < A.ntri; t++) {
    const int i = tri_i[t], j = tri_j[t];
    ent[t] = (int)((unsigned)((i << 8) | j) | ((unsigned)S.lanes[i].d_pos << 16) | ((unsigned)S.lanes[j].d_pos << 20));
  }
  A.o_ent = push_tbl(ent);
}

// packed pair records for the broad phase: pairs with a static world geom first (the model lists them first:
// body-pair order, world body = 0), padded to whole rounds of 64, then the pairs between moving geoms.
//   world pair:  moving centre | world centre << 8 | (world geom is geom1) << 16 | valid << 17
//                bound = margin + rbound(moving geom) [+ radius of a static capsule; + rbound of other static shapes]
//   moving pair: c1 | c2 << 8 | valid << 17;  bound = margin + rbound1 + rbound2
// bounds are rounded up in float: the broad phase may only over-include
int AuxBuilder::pair_records() {
  int nwp = 0;
  while (nwp < m->npair && (gbody[SUMO_I(m, pair_geom1)[nwp]] == 0 || gbody[SUMO_I(m, pair_geom2)[nwp]] == 0)) nwp++;
  for (int p = nwp; p < m->npair; p++)
    if (gbody[SUMO_I(m, pair_geom1)[p]] == 0 || gbody[SUMO_I(m, pair_geom2)[p]] == 0)
      FAIL(-23, "collision pair %d: pairs with a world geom must precede the others", p);
  const int WR = (nwp + WAVE - 1) / WAVE, AR = (m->npair - nwp + WAVE - 1) / WAVE;
  A.nwp = nwp; A.wrounds = WR; A.arounds = AR;
  S.pair_rec.assign((size_t)(WR + AR) * WAVE, 0);
  S.pair_bound.assign((size_t)(WR + AR) * WAVE, 0.0f);
  auto up = [](double bound) {
    float bf = (float)bound;
    while ((double)bf < bound) bf = nextafterf(bf, INFINITY);
    return nextafterf(bf, INFINITY);
  };
  for (int p = 0; p < m->npair; p++) {
    int g1 = SUMO_I(m, pair_geom1)[p], g2 = SUMO_I(m, pair_geom2)[p];
    const double margin = SUMO_F(m, pair_margin)[p];
    if (p < nwp) {
      if (gbody[g1] == 0 && gbody[g2] == 0) continue;   // static-static: never collides (slot stays invalid)
      const int w1 = gbody[g1] == 0, gw = w1 ? g1 : g2, ga = w1 ? g2 : g1, tw = gtype[gw];
      double bound = margin + SUMO_F(m, geom_rbound)[ga];
      if (tw == SUMO_GEOM_CAPSULE || tw == SUMO_GEOM_CYLINDER) bound += SUMO_F(m, geom_size)[3 * gw];
      else if (tw != SUMO_GEOM_BOX && tw != SUMO_GEOM_PLANE) bound += SUMO_F(m, geom_rbound)[gw];
      S.pair_rec[p] = cen_of_geom[ga] | (cen_of_geom[gw] << 8) | (w1 << 16) | (1 << 17);
      S.pair_bound[p] = up(bound);
    } else {
      const int sl = WR * WAVE + (p - nwp);
      S.pair_rec[sl] = cen_of_geom[g1] | (cen_of_geom[g2] << 8) | (1 << 17);
      S.pair_bound[sl] = up(margin + SUMO_F(m, geom_rbound)[g1] + SUMO_F(m, geom_rbound)[g2]);
    }
  }
  return 0;
}

static void build_layout_with(Scene& S, const SceneOptions& opt, int jb_extra) {
  const sumo_model_t* m = &S.hm;
  Layout& L = S.L;
  int nq = m->nq, nv = m->nv, nb = m->nbody, nj = m->njnt, nu = m->nu;
  L.ld = nv | 1;
  int nhinge = 0;
  for (int j = 0; j < nj; j++) if (SUMO_I(m, jnt_type)[j] == SUMO_JNT_HINGE) nhinge++;
  // Ant-vs-Ant: 18 contact records (the soaks and the zoo play never saw more than 14) instead of 24: the 1 KB goes to the contact-Jacobian pool
  // (build_layout: 29 halves instead of 24 -- 14 contacts between two moving bodies fit), which is what overflowed a few times per 10^8 forwards
  L.maxcon = nv <= 28 ? 18 : (nv <= 36 ? 32 : 40);
  if (opt.maxcon > 0) L.maxcon = opt.maxcon;
  { int cap = 16 * (nv <= 36 ? 2 : 3); if (L.maxcon > cap) L.maxcon = cap; }  // contact rows per lane held in registers by the line search (newton_solve RPL)
  L.maxefc = 4 * L.maxcon + 2 * nhinge;
  L.warm_mode = opt.warm_mode; L.force_dense = opt.force_dense;
  int o = 0;
  auto take = [&](int n) { int r = o; o += n; return r; };
  L.qpos = take(nq); L.qvel = take(nv); L.warm = take(nv); L.ctrl = take(nu);
  L.x0 = 0; L.accv = 0; L.acca = 0; L.tmpv = take(nv);
  // kinematic data needed until the mass matrix is built (com, cinert -> crb, cdof); the packed Hessian aliases it
  const int nc = S.aux.nc;
  const int ntri = nv * (nv + 1) / 2;
  int kin0 = o;
  L.com = take(3 * m->nagent); L.cinert = take(10 * nb); L.cdof = take(6 * nv);
  L.H = kin0;
  if (o - kin0 < ntri) o = kin0 + ntri;
  const int hsize = o - kin0;
  // centre positions / axes: bodies (rewritten every forward) then world geoms (static)
  L.xipos = take(3 * nc); L.gaxis = take(3 * nc);
  L.stat_d = take(SUMO_STAT_LDS ? S.aux.n_stat_d : 0);
  {
    int nv0 = SUMO_I(m, agent_nv)[0], nv1 = SUMO_I(m, agent_nv)[1];
    int mx = nv0 > nv1 ? nv0 : nv1;
    L.mld = mx | 1;
    L.d1 = SUMO_I(m, agent_dofadr)[1];
    L.msize = (nv0 + nv1) * L.mld;
  }
  {  // shape tree_factor_solve relies on: two agents, each a free joint (6 dofs) + legs of (hip, ankle), bases even
    const int* dpar = SUMO_I(m, dof_parentid);
    int ok = m->nagent == 2 && SUMO_I(m, agent_dofadr)[0] == 0 && SUMO_I(m, agent_nv)[0] + SUMO_I(m, agent_nv)[1] == nv;
    for (int g = 0; ok && g < 2; g++) {
      int B = SUMO_I(m, agent_dofadr)[g], n = SUMO_I(m, agent_nv)[g];
      if ((B & 1) || n < 6 || ((n - 6) & 1)) { ok = 0; break; }
      if (dpar[B] != -1) ok = 0;
      for (int k = 1; ok && k < 6; k++) if (dpar[B + k] != B + k - 1) ok = 0;
      for (int d = B + 6; ok && d < B + n; d += 2) if (dpar[d] != B + 5 || dpar[d + 1] != d) ok = 0;
    }
    if (14 * nv > hsize) ok = 0;   // exchange buffers of the tree solver live in the Hessian region
    L.tree_ok = ok;
    if (opt.no_tree) L.tree_ok = 0;
  }
  L.qsm = take(nv); L.asmo = take(nv); L.Ma = 0; L.grad = 0;
  L.search = take(nv); L.bias = L.search;   // the bias force is consumed (into qsm) before the solver writes its search direction
  L.Mv = 0; L.x = take(nv); L.dlim = take(nv); L.cmask = take(nv); L.stash = take(12);   // + the fused rollout's ticket (env, step) and the step's reward inputs / episode record for its post phase
  // contact records live from the narrow phase to the Jacobian build only: they borrow the mass matrix's storage
  if (L.msize < 14 * L.maxcon) L.msize = 14 * L.maxcon;
  if (L.msize < 12 * nb) L.msize = 12 * nb;      // ... and so do the velocity-pass temporaries (abuf, cfrc), see below
  L.M = take(L.msize);
  L.cond = L.M;
  // body frames / joint anchors / RNE temporaries are dead before the contact Jacobians are written: same storage
  {
    // pool of Jacobian halves (3 rows x 8 slots, one half per moving body of a contact): room for maxcon contacts with the
    // world, or half as many between two moving bodies -- more where the frames' storage leaves space anyway
    int need = 7 * nb + 6 * nj;
    L.jbcap = L.maxcon;
    if ((need - 16) / 24 > L.jbcap) L.jbcap = (need - 16) / 24;
    L.jbcap += jb_extra;
    if (opt.jbcap > 0) L.jbcap = opt.jbcap;
    int jb0 = o, jbsz = 24 * L.jbcap + 16;
    L.Jb = take(jbsz > need ? jbsz : need);
    int q = jb0;
    L.xpos = q; q += 3 * nb; L.xquat = q; q += 4 * nb; L.xanchor = q; q += 3 * nj; L.xaxis = q; q += 3 * nj;
    // velocity-pass temporaries (dead before the narrow phase writes contact records there): the mass matrix's storage
    L.abuf = L.M; L.cfrc = L.M + 6 * nb;
  }
  L.cpar = take(L.maxcon); L.cW = take(5 * L.maxcon);
  L.cp = take(3 * L.maxcon);
  // row arrays hold the contact rows only (4 per contact); the limit rows live in the dof-indexed slots limD / limA
  L.jar = take(4 * L.maxcon); L.D = take(L.maxcon); L.aref = take(4 * L.maxcon);
  L.nhinge = nhinge; L.limD = take(2 * nhinge); L.limA = take(2 * nhinge);
  // queue of broad-phase survivors (ints, inside jar / aref); drained by the narrow phase before it can overflow
  L.maxcand = 8 * L.maxcon >= 192 ? 192 : (8 * L.maxcon) / WAVE * WAVE;
  L.i_base = o;
  int io = 0;
  auto itake = [&](int n) { int r = io; io += n; return r; };
  L.con_b = itake(4 * L.maxcon);
  L.stat_i = itake(SUMO_STAT_LDS ? S.aux.n_stat_i : 0);
  L.b_dofidx = io * 4;
  L.total_bytes = o * 8 + io * 4 + 16 * L.maxcon;
}
// The LDS a wave slot leaves unused at the scene's residency (160 KB / waves per CU - the env record) goes to the contact-Jacobian
// pool: a contact between two moving bodies takes two halves, and wrestling Spiders overflowed a pool of `maxcon` halves about twice
// per million env steps (counted in `dropped`).  Ant-vs-Ant has 32 B to spare (8 x 20 448 B = 163 584 of 163 840): unchanged.
static void build_layout(Scene& S, const SceneOptions& opt) {
  build_layout_with(S, opt, 0);
  const int lds_cu = 160 * 1024, slots = lds_cu / S.L.total_bytes;
  if (slots < 1 || opt.jbcap_set) return;
  const int budget = lds_cu / slots / 1280 * 1280;   // LDS is allocated in granules of 1280 B on gfx950
  int extra = (budget - S.L.total_bytes) / (24 * 8);
  if (extra > S.L.maxcon) extra = S.L.maxcon;        // (a pool of 2 x maxcon halves can never overflow)
  if (extra <= 0) return;
  build_layout_with(S, opt, extra);
  if (lds_cu / S.L.total_bytes != slots) build_layout_with(S, opt, 0);   // (cannot happen: the growth was sized to fit)
}

// The two role words of every lane (LaneRec::role0 / role1), packed from the records build_aux filled; after build_layout, whose
// tree_ok decides whether the kernels derive chain elements from the words.  Nothing is truncated: a value that does not fit its
// field, or a scene in which a derived quantity differs from the model's, fails creation.
static int build_lane_roles(Scene& S) {
  const sumo_model_t* m = &S.hm;
  const char* bad = nullptr; int bad_lane = 0; long bad_val = 0;
  int nfree = 0;   // free joints before joint l
  for (int l = 0; l < WAVE; l++) {
    LaneRec& K = S.lanes[l];
    unsigned w[2] = {0u, 0u};
    auto put = [&](int wi, int lo, int n, long v, const char* what) {
      if ((v < 0 || v >= (1L << n)) && !bad) { bad = what; bad_lane = l; bad_val = v; }
      w[wi] |= ((unsigned)v & ((1u << n) - 1u)) << lo;
    };
    const int hinge = l < m->nbody && K.b_jnt >= 0 && !K.b_isfree;
    put(0, ROLE0_LEVEL1, K.b_level + 1, "b_level");
    put(0, ROLE0_AGENT, K.b_agent, "b_agent");
    put(0, ROLE0_ISFREE, K.b_isfree, "b_isfree");
    put(0, ROLE0_HINGE, hinge, "b_hinge");
    put(0, ROLE0_PARENT, l >= 1 ? K.b_parent : 0, "b_parent");
    put(0, ROLE0_NCHILD, K.b_nchild, "b_nchild");
    put(0, ROLE0_CHAIN_LEN, K.b_chain_len, "b_chain_len");
    put(0, ROLE0_BCHAIN_LEN, K.b_bchain_len, "b_bchain_len");
    put(0, ROLE0_QADR, K.b_qadr, "b_qadr");
    put(1, ROLE1_LDOF, K.b_chain_len > 0 ? BYTE_OF(K.b_chain, K.b_chain_len - 1) : 0, "b_chain (last dof)");
    put(1, ROLE1_HID1, l < m->nv ? K.d_hid + 1 : 0, "d_hid");
    put(1, ROLE1_DPOS, K.d_pos, "d_pos");
    put(1, ROLE1_DBODY, K.d_body, "d_body");
    if (l < m->njnt) {
      if (K.jt_type != SUMO_JNT_FREE && K.jt_type != SUMO_JNT_HINGE) FAIL(-26, "joint %d has type %d; the engine supports free joints and hinges", l, K.jt_type);
      const int jh = K.jt_type == SUMO_JNT_HINGE;
      put(0, ROLE0_JT_HINGE, jh, "jt_type");
      put(0, ROLE0_JT_LIMITED, K.jt_limited, "jt_limited");
      put(0, ROLE0_JT_AGENT, K.jt_agent, "jt_agent");
      put(1, ROLE1_JT_NFREE, nfree, "free joints before the joint");
      put(1, ROLE1_JT_BODY, K.jt_body, "jt_body");
      if (K.jt_dadr != l + 5 * nfree || K.jt_qadr != l + 6 * nfree || (jh && K.jt_hid != l - nfree))
        FAIL(-26, "joint %d: dof address %d / qpos address %d / hinge index %d do not follow from %d free joints before it", l, K.jt_dadr,
             K.jt_qadr, K.jt_hid, nfree);
      if (!jh) nfree++;
    }
    if (bad) FAIL(-26, "lane %d: %s = %ld does not fit its field of the lane role words", bad_lane, bad, bad_val);
    if (S.L.tree_ok && l >= 1 && l < m->nbody) {   // what the tree-shaped velocity pass derives instead of reading b_chain / b_chain_own
      const int len = K.b_chain_len, ld = len > 0 ? BYTE_OF(K.b_chain, len - 1) : 0, B = K.b_agent ? S.L.d1 : 0;
      int ok = len >= 6 && len <= 8;
      for (int p = 0; ok && p < len; p++) {
        const int want = p < 6 ? B + p : (len > 7 ? ld - 7 + p : ld);
        if (BYTE_OF(K.b_chain, p) != want) ok = 0;
      }
      const unsigned own = (K.b_isfree ? 0x3Fu : 0u) | (hinge && len > 6 ? 1u << (len - 1) : 0u);
      if (!ok || K.b_chain_own != own || (hinge && len <= 6))
        FAIL(-26, "body %d: its dof chain is not the root's six dofs, then hip and ankle, owned as its joint says", l);
    }
    K.role0 = w[0]; K.role1 = w[1];
  }
  return 0;
}

// the integer members of the compiled model view (header dims, then the int / float table offsets in SUMO_*_TABLES order)
static int model_ints(const sumo_model_t* m, int32_t* out) {
  int n = 0;
  out[n++] = m->nq; out[n++] = m->nv; out[n++] = m->nu; out[n++] = m->nbody; out[n++] = m->njnt; out[n++] = m->ngeom; out[n++] = m->npair;
  out[n++] = m->nagent; out[n++] = m->frame_skip; out[n++] = m->timestep_limit;
#define X(name, len) out[n++] = m->o_##name;
  SUMO_INT_TABLES(X)
  SUMO_FLT_TABLES(X)
#undef X
  return n;
}

// The last stage of a preparation, what only the whole scene can answer: which kernel variants run it, whether its constraint rows
// fit the registers, and the strides of its per-env records.
static int finish_scene(Scene& S, const SceneOptions& opt) {
  {   // static kernel variants only when the runtime Layout IS the compile-time table (SUMO_STATIC_LAYOUT=0 switches them off)
    static_assert(sizeof(Layout) % sizeof(int) == 0, "Layout is all ints");
    int32_t mi[160];
    const int nmi = model_ints(&S.hm, mi);
    auto same = [&](const int* kl, size_t nl, const int* km, size_t nm_, const int* ka, size_t na) {
      return nl == sizeof(Layout) && memcmp(&S.L, kl, nl) == 0 && nm_ == nmi * sizeof(int) && memcmp(mi, km, nm_) == 0 &&
             na == AUX_NINTS * sizeof(int) && memcmp(&S.aux.ndepth, ka, na) == 0;
    };
    S.static_layout = 0;      // 1: Ant-vs-Ant, 2: Spider-vs-Spider (the scenes of csrc/layout_static.h), 0: runtime-Layout variants
    if (opt.static_layout) {
      if (same(kLayoutAntAnt, sizeof(kLayoutAntAnt), kModelAntAnt, sizeof(kModelAntAnt), kAuxAntAnt, sizeof(kAuxAntAnt))) S.static_layout = 1;
      else if (same(kLayoutSpiderSpider, sizeof(kLayoutSpiderSpider), kModelSpiderSpider, sizeof(kModelSpiderSpider), kAuxSpiderSpider, sizeof(kAuxSpiderSpider)))
        S.static_layout = 2;
    }
  }
  if (S.L.maxefc > WAVE * (S.hm.nv <= 28 ? 2 : 4)) FAIL(-24, "maxefc %d exceeds the rows a lane keeps in registers", S.L.maxefc);
  const sumo_model_t* m = &S.hm;
  int od = 0, ad = 0;
  for (int a = 0; a < m->nagent; a++) {
    int o = SUMO_I(m, agent_nq)[a] + SUMO_I(m, agent_nv)[a] + 6 * SUMO_I(m, agent_nbody)[a] + 14;
    if (o > od) od = o;
    if (SUMO_I(m, agent_nu)[a] > ad) ad = SUMO_I(m, agent_nu)[a];
  }
  S.obs_stride = od; S.act_stride = ad;
  S.state_stride = (m->nq + 2 * m->nv + 2 + 15) & ~15;
  return 0;
}

// The Newton loop's gradient test D(gn) = (scale * sqrt(gn) < tol) as a threshold on gn, the squared gradient norm: with a correctly
// rounded sqrt and scale >= 0, D is non-increasing over gn >= 0, so D(gn) == (gn <= G) for G the largest double with D(G) true (-1 where
// there is none; gn is a sum of squares, never below +0).  NaN and +inf fail both forms.  Found by bisection over the bit patterns of the
// non-negative finite doubles, which are ordered like their values.
static double grad_threshold(double scale, double tol) {
  auto D = [&](uint64_t bits) { double g; memcpy(&g, &bits, sizeof g); volatile double s = sqrt(g); volatile double p = scale * s; return p < tol; };
  uint64_t lo = 0, hi = 0x7FEFFFFFFFFFFFFFull;   // +0 .. DBL_MAX
  if (!D(lo)) return -1.0;
  while (lo < hi) {   // invariant: D(lo) true
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (D(mid)) lo = mid; else hi = mid - 1;
  }
  double g; memcpy(&g, &lo, sizeof g);
  return g;
}
static double newton_scale(const sumo_model_t* m) { return 1.0 / (SUMO_F(m, opt)[SUMO_OPT_MEANINERTIA] * (m->nv > 1 ? m->nv : 1)); }   // newton_solve's `scale`

// The one preparation of a scene from a model blob, in stages; a caller stops after the stage it needs, and a scene that fails a
// later stage still answers for the earlier ones.  Host only.
enum SceneStage { SCENE_AUX, SCENE_LAYOUT, SCENE_ROLES, SCENE_CHECKED };
static int prepare_scene(Scene& S, const void* blob, size_t nbytes, SceneStage upto) {
  const SceneOptions opt = SceneOptions::from_env();
  S.blob.assign((const char*)blob, (const char*)blob + nbytes);
  if (int rc = sumo_model_parse(&S.hm, S.blob.data(), nbytes)) FAIL(-4, "malformed model blob (%d)", rc);
  if (int rc = build_aux(S, opt)) return rc;             // aux tables, lane records, pair records
  S.grad_thresh = grad_threshold(newton_scale(&S.hm), SUMO_F(&S.hm, opt)[SUMO_OPT_TOLERANCE]);
  if (upto == SCENE_AUX) return 0;
  build_layout(S, opt);
  if (upto == SCENE_LAYOUT) return 0;
  if (int rc = build_lane_roles(S)) return rc;           // after the layout: its tree_ok decides what the words must carry
  if (upto == SCENE_ROLES) return 0;
  return finish_scene(S, opt);
}

