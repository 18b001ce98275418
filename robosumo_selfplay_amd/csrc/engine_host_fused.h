// engine_host_fused.h -- the fused launches: EnvBuffers .. rollout_launch, the family checks, the zoo tables, the seventeen fused entry points.
// Not in a shard object.
// A part of the sumo_engine.hip translation unit, not a stand-alone header: no includes of its own.

// the env-side buffers of sumo_step, as every fused entry point receives them
struct EnvBuffers {
  float *actions, *obs;
  double* info;
  uint8_t* done;
  double *ep_r, *ep_dr;
  int32_t* ep_l;
};
static int check_launch_args(sumo_engine* E, const void* launch, const EnvBuffers& b) {
  if (!E || !launch || !b.actions || !b.obs || !b.info || !b.done || !b.ep_r || !b.ep_dr || !b.ep_l) FAIL(-1, "bad arguments");
  return 0;
}

// the instantiation of sumo_rollout_kernel for `policy`, from a table of all of them
typedef void (*RolloutKernel)(const Params*, RolloutLaunch);
template <int NV, int SL, int... POLICY>
static RolloutKernel rollout_kernel(int policy, std::integer_sequence<int, POLICY...>) {
  static const RolloutKernel table[] = {sumo_rollout_kernel<NV, POLICY, SL>...};
  return table[policy];
}

// common tail of the fused entry points: scheduler state, persistent grid, launch
static int rollout_launch(sumo_engine* E, const RolloutArgs& r, int policy, const EnvBuffers& b, void* stream) {
  RolloutLaunch rl;
  rl.a = base_args(E);
  StepArgs& a = rl.a;
  a.actions = b.actions; a.obs = b.obs; a.info = b.info; a.done = b.done; a.ep_r = b.ep_r; a.ep_dr = b.ep_dr; a.ep_l = b.ep_l;
  rl.r = r;
  rl.r.prof = E->d_trace;   // development: sumo_debug_trace(stamps) switches the per-wave phase clock on
  hipStream_t st_ = (hipStream_t)stream;
  if (!E->d_rsched) HIPCHK(E->d_rsched.alloc((size_t)(2 + E->N)));
  HIPCHK(hipMemsetAsync(E->d_rsched, 0, (size_t)(2 + E->N) * sizeof(int), st_));
  rl.r.sched = E->d_rsched;
  if (r.K >= 65536) FAIL(-5, "K = %d: at most 65535 steps per fused launch", r.K);
  E->rollout_seq++;
  a.seq_base = (int)((E->rollout_seq & 0x7FFFu) << 16);
  a.abort_flag = E->d_rsched + 1;
  a.dbg_fault_env = E->dbg_fault_env;
  E->rollout_stream = st_;
  E->rollout_tickets = (long long)E->N * r.K;
  // persistent waves: as many as the chip holds at this kernel's LDS footprint (8 per CU at most: two per SIMD)
  int slots = (int)((size_t)160 * 1024 / (size_t)E->L.total_bytes);
  if (slots > 4 * SUMO_WPE_OF(E->hm.nv)) slots = 4 * SUMO_WPE_OF(E->hm.nv);
  if (slots < 1) slots = 1;
  if (E->num_cus <= 0) {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, E->device));
    E->num_cus = prop.multiProcessorCount;
  }
  long long nw = (long long)slots * E->num_cus;
  if (nw > (long long)E->N) nw = E->N;   // more waves than envs would only wait on each other's steps
  dim3 g_((unsigned)nw), b_(WAVE);
  size_t lds_ = (size_t)E->L.total_bytes;
  if (!for_engine_variant(E, [&](auto nvc_, auto slc_) {
        constexpr int NV = decltype(nvc_)::value, SL = decltype(slc_)::value;
        const RolloutKernel kernel = rollout_kernel<NV, SL>(policy, std::make_integer_sequence<int, SUMO_N_POLICY>{});
        hipLaunchKernelGGL(kernel, g_, b_, lds_, st_, E->d_params, rl);
      }))
    FAIL(-19, "no kernel variant for nv=%d", E->hm.nv);
  HIPCHK(hipGetLastError());
  return 0;
}

// scene checks shared by the entry points; returns the observation / action width through od / ad
static int rollout_scene(sumo_engine* E, int T, int Ntot, int env_offset, int s0, int K, int* od, int* ad) {
  const sumo_model_t* m = &E->hm;
  if (E->cfrc_mode) FAIL(-12, "cfrc_mode rne_post fills the observations in a second launch per step: use sumo_step (the fused rollout evaluates the policies inside its launch)");
  const int* anq = SUMO_I(m, agent_nq); const int* anv = SUMO_I(m, agent_nv); const int* anb = SUMO_I(m, agent_nbody);
  const int* anu = SUMO_I(m, agent_nu);
  const int od0 = anq[0] + anv[0] + 6 * anb[0] + 14, od1 = anq[1] + anv[1] + 6 * anb[1] + 14;
  if (od0 != od1 || anu[0] != anu[1]) FAIL(-3, "fused rollout needs a homogeneous match-up (one observation / action space for both sides, runner.py:14-16)");
  if (T < 1 || K < 1 || s0 < 0 || s0 + K > T) FAIL(-5, "steps [%d, %d) outside the rollout buffers (T = %d)", s0, s0 + K, T);
  if (env_offset < 0 || env_offset + E->N > Ntot) FAIL(-6, "envs [%d, %d) outside the rollout buffers (N = %d)", env_offset, env_offset + E->N, Ntot);
  *od = od0; *ad = anu[0];
  return 0;
}

static int check_dims(int ob_dim, int ac_dim, int od, int ad) {
  if (ob_dim != od || ac_dim != ad || ac_dim > PT_MAXA) FAIL(-4, "ob_dim %d / ac_dim %d do not match the scene (%d / %d)", ob_dim, ac_dim, od, ad);
  return 0;
}

// what the in-wave recurrent evaluation is built for: the nets `learn(network='lstm')` trains (policy-zoo LSTM nets carry an
// observation filter, an embedding and the other gate order: they play as agent 1 of the match modes 6 / 7, zoo_lstm_act)
static int check_lstm_shape(const ppo_lstm_net& n, const char* what) {
  if (n.hidden != 128 || n.gate_order != PPO_LSTM_GATES_IFOU || n.emb_w || n.emb_dim != 0 || n.obs_mean || n.obs_invstd)
    FAIL(-9, "fused recurrent %s: hidden 128, gate order i,f,o,u, no embedding, no observation filter (got hidden %d, order %d, emb %d)", what, n.hidden, n.gate_order, n.emb_dim);
  return 0;
}

// MLP phases: x [2][XS] and the two hidden tiles go where the mass matrix lives between two steps.  valu_nets > 0 (modes 0 and 2:
// that many trunks in one pass of mlp_rows_valu): x rows and the activation rows [valu_nets][2][PT_VS] 16-byte aligned for the
// 128-bit LDS reads, the x rows zero-padded to a multiple of four columns
static int place_mlp_scratch(sumo_engine* E, int ob_dim, int ac_dim, RolloutArgs& r, int valu_nets = 0) {
  r.XS = valu_nets ? (ob_dim + 3) & ~3 : x_stride(ob_dim); r.L = make_layout(ob_dim, ac_dim);
  r.lds_off = valu_nets ? (E->L.M + 1) & ~1 : E->L.M;
  const size_t need = (size_t)(2 * r.XS + (valu_nets ? valu_nets * 2 * PT_VS : 4 * PT_HS)) * sizeof(float);
  const size_t have = (size_t)(E->L.M + E->L.msize - r.lds_off) * sizeof(double);
  if (need > have) FAIL(-8, "policy scratch (%zu B) does not fit the mass-matrix region (%zu B)", need, have);
  return 0;
}

// LSTM phases: x [2][XS] and `rows` rows of 128 floats.  Between two steps of an env nothing from the mass matrix to the end of the
// float64 area is live (contact records, Jacobian pool and row arrays are rebuilt by every forward): the rows go there, 16-byte
// aligned for the 128-bit LDS reads
static int place_lstm_scratch(sumo_engine* E, int od, int rows, RolloutArgs& r) {
  r.XS = (od + 3) & ~3;
  r.lds_off = (E->L.M + 1) & ~1;
  const size_t need = (size_t)(2 * r.XS + rows * 128) * sizeof(float), have = (size_t)(E->L.i_base - r.lds_off) * sizeof(double);
  if (E->L.ctrl >= E->L.M || E->L.stash >= E->L.M || need > have) FAIL(-8, "policy scratch (%zu B) does not fit the per-step LDS area (%zu B)", need, have);
  return 0;
}

// the fields sumo_rollout and sumo_rollout_lstm share
template <class RO>
static bool rollout_buffer_missing(const RO* ro) {
  return !ro->noise0 || !ro->noise1 || !ro->obs || !ro->act || !ro->rew || !ro->val || !ro->nlp || !ro->onlp || !ro->done || !ro->ep_done ||
         !ro->ep_r || !ro->ep_l;
}
template <class RO>
static void copy_rollout_fields(RolloutArgs& r, const RO* ro) {
  r.noise0 = ro->noise0; r.noise1 = ro->noise1;
  r.obs = ro->obs; r.act = ro->act; r.rew = ro->rew; r.val = ro->val; r.nlp = ro->nlp; r.onlp = ro->onlp; r.done = ro->done;
  r.ep_done = ro->ep_done; r.ep_r = ro->ep_r; r.ep_l = ro->ep_l; r.alpha = ro->alpha;
  r.T = ro->T; r.Ntot = ro->Ntot; r.env_offset = ro->env_offset; r.s0 = ro->s0; r.K = ro->K;
}

// the fields sumo_match and sumo_match_lstm share: their checks (`name`: the struct in the messages) and the copy
template <class MO>
static int check_match_buffers(const MO* mo, const char* name) {
  if (!mo->idx0 || !mo->idx1 || !mo->score) FAIL(-2, "%s: missing buffer", name);
  if (!mo->noise0 != !mo->noise1) FAIL(-2, "%s: noise0 and noise1 are both given (stochastic play) or both NULL (deterministic)", name);
  return 0;
}
template <class MO>
static int check_match_counts(const MO* mo) {
  if (mo->nsnap < 1) FAIL(-7, "nsnap %d: the snapshot table needs at least one entry", mo->nsnap);
  if (mo->quota < 0) FAIL(-9, "quota %d", mo->quota);
  return 0;
}
template <class MO>
static void copy_match_fields(RolloutArgs& r, const MO* mo, int N) {
  r.idx0 = mo->idx0; r.idx1 = mo->idx1; r.score = mo->score; r.nsnap = mo->nsnap; r.quota = mo->quota;
  r.noise0 = mo->noise0; r.noise1 = mo->noise1;
  r.T = mo->T; r.Ntot = N; r.s0 = mo->s0; r.K = mo->K;
}

// ---- what the fused entry points share.  check_*: a family's buffer, scene and dimension checks, in the order every mode of the
// family reports them (a zoo mode's own count checks follow in the entry point); begin_*: device and the family's fields, into a
// zeroed RolloutArgs.  `zoo`: the entry point's name in a zoo mode (which refuses the fields that only play without a zoo), else NULL ----
// MLP(64,64) learner (modes 0, 4, 8, 11)
static int check_mlp_rollout(sumo_engine* E, const sumo_rollout* ro, const char* zoo, bool league, int* od, int* ad) {
  if (!ro->learner_params || (!zoo && !ro->opponent_params) || rollout_buffer_missing(ro)) FAIL(-2, "sumo_rollout: missing buffer");
  if (zoo && !league && ro->opponent_params) FAIL(-2, "%s: opponent_params must be NULL (the opponents are the zoo table's nets)", zoo);
  if (league && (ro->opponent_params || ro->opponent_index))
    FAIL(-2, "%s: opponent_params and opponent_index must be NULL (the opponents are the league's nets, selected per tile by tile_entry_dev)", zoo);
  if (int rc = rollout_scene(E, ro->T, ro->Ntot, ro->env_offset, ro->s0, ro->K, od, ad)) return rc;
  return check_dims(ro->ob_dim, ro->ac_dim, *od, *ad);
}
static int begin_mlp_rollout(sumo_engine* E, const sumo_rollout* ro, RolloutArgs& r) {
  HIPCHK(hipSetDevice(E->device));
  r.learner = ro->learner_params; r.opponent = ro->opponent_params; r.opp_idx = ro->opponent_index;
  copy_rollout_fields(r, ro);
  return 0;
}

// LSTM(128) learner (modes 1, 9, 10, 12).  nzoo: the size of the zoo mode's table or league.  begin_lstm_rollout also places the
// scratch: x [2][XS] and `rows` rows of 128 floats
static int check_lstm_rollout(sumo_engine* E, const sumo_rollout_lstm* ro, const char* zoo, int nzoo, int* od, int* ad) {
  if (!ro->learner || !ro->state0 || (!zoo && (!ro->opponents_dev || !ro->state1)) || rollout_buffer_missing(ro)) FAIL(-2, "sumo_rollout_lstm: missing buffer");
  if (zoo && (ro->opponents_dev || ro->state1))
    FAIL(-2, "%s: opponents_dev and state1 must be NULL (the opponents are the zoo table's nets, agent 1's state is the table's)", zoo);
  if (int rc = rollout_scene(E, ro->T, ro->Ntot, ro->env_offset, ro->s0, ro->K, od, ad)) return rc;
  const ppo_lstm_net& n = *ro->learner;
  if (int rc = check_dims(n.ob_dim, n.ac_dim, *od, *ad)) return rc;
  if (int rc = check_lstm_shape(n, "rollout")) return rc;
  if (!n.wx || !n.wh || !n.b || !n.head_w || !n.head_b || !n.logstd || !n.vf_w || !n.vf_b) FAIL(-10, "learner net: missing weights");
  if (!zoo && ro->npool < 1) FAIL(-7, "npool %d", ro->npool);
  if (zoo && ro->npool != nzoo) FAIL(-7, "npool %d must equal the zoo table's nzoo %d", ro->npool, nzoo);
  if (ro->tile_net_dev && ((ro->env_offset & 15) || (E->N & 15)))
    FAIL(-11, "a %s per 16-env tile needs env_offset (%d) and the env count (%d) to be multiples of 16", zoo ? "zoo net" : "snapshot", ro->env_offset, E->N);
  return 0;
}
static int begin_lstm_rollout(sumo_engine* E, const sumo_rollout_lstm* ro, int od, int rows, RolloutArgs& r) {
  HIPCHK(hipSetDevice(E->device));
  r.lnet = *ro->learner; r.onets = ro->opponents_dev; r.tile_net = ro->tile_net_dev; r.st0 = ro->state0; r.st1 = ro->state1;
  copy_rollout_fields(r, ro);
  return place_lstm_scratch(E, od, rows, r);
}
// the rows of a recurrent learner's zoo modes: zero row, agent 0's previous latent, two new latents, which the zoo net's hidden
// tiles / cell rows reuse
constexpr int LSTM_ZOO_ROWS = 4;
static_assert(4 * PT_HS <= LSTM_ZOO_ROWS * 128, "modes 9 / 12: the zoo trunk's two hidden tiles [2][PT_HS] go where the learner's latent rows were");

// MLP(64,64) checkpoints as agent 0, or on both sides (modes 2, 5, 6): nothing of a mode's own comes between checks and fields
static int begin_mlp_match(sumo_engine* E, const sumo_match* mo, int* od, int* ad, RolloutArgs& r) {
  if (!mo->params) FAIL(-2, "sumo_match: missing buffer");
  if (int rc = check_match_buffers(mo, "sumo_match")) return rc;
  if (int rc = rollout_scene(E, mo->T, E->N, 0, mo->s0, mo->K, od, ad)) return rc;
  if (int rc = check_dims(mo->ob_dim, mo->ac_dim, *od, *ad)) return rc;
  if (int rc = check_match_counts(mo)) return rc;
  HIPCHK(hipSetDevice(E->device));
  r.snaps = mo->params;
  copy_match_fields(r, mo, E->N);
  return 0;
}

// LSTM(128) checkpoints (modes 3, 7, 13, 14), with the scratch: x [2][XS] | `rows` rows of 128 floats (previous latent | new latent)
static int begin_lstm_match(sumo_engine* E, const sumo_match_lstm* mo, const char* zoo, int* od, int* ad, RolloutArgs& r, int rows = 2) {
  if (!mo->proto || !mo->nets_dev) FAIL(-2, "sumo_match_lstm: missing buffer");
  if (!mo->state0 || (!zoo && !mo->state1)) FAIL(-2, "sumo_match_lstm: missing state buffer (%s)", zoo ? "state0" : "state0 / state1");
  if (zoo && mo->state1) FAIL(-2, "%s: state1 must be NULL (agent 1's state is the zoo table's state)", zoo);
  if (int rc = check_match_buffers(mo, "sumo_match_lstm")) return rc;
  if (int rc = rollout_scene(E, mo->T, E->N, 0, mo->s0, mo->K, od, ad)) return rc;
  const ppo_lstm_net& n = *mo->proto;
  if (int rc = check_dims(n.ob_dim, n.ac_dim, *od, *ad)) return rc;
  if (int rc = check_lstm_shape(n, "matches")) return rc;   // the nets sumo_rollout_steps_lstm plays
  if (!n.wx || !n.wh || !n.b || !n.head_w || !n.head_b || !n.logstd) FAIL(-10, "prototype net: missing weights");
  if (int rc = check_match_counts(mo)) return rc;
  HIPCHK(hipSetDevice(E->device));
  r.lnet = n; r.onets = mo->nets_dev; r.st0 = mo->state0; r.st1 = mo->state1;
  copy_match_fields(r, mo, E->N);
  return place_lstm_scratch(E, *od, rows, r);
}
// the rows of modes 13 / 14: the recurrent side's two latent rows, then the two hidden tiles of the MLP / zoo trunk in their place
constexpr int LSTM_MLP_MATCH_ROWS = 3;
static_assert(4 * PT_HS <= LSTM_MLP_MATCH_ROWS * 128 && 2 * 128 <= LSTM_MLP_MATCH_ROWS * 128, "modes 13 / 14: the larger of the latent rows and the hidden tiles [2][PT_HS] twice");

// ---- the zoo tables: checks, then RolloutArgs::zm / zl ----
static int place_zoo_mlp_table(RolloutArgs& r, const sumo_zoo_mlp* z, int od, int ad) {
  if (!z->params || !z->filt) FAIL(-2, "sumo_zoo_mlp: missing buffer (params / filt)");
  if (z->nzoo < 1) FAIL(-7, "nzoo %d: the zoo table needs at least one entry", z->nzoo);
  if (z->ob_dim < 1 || z->ob_dim > od)
    FAIL(-4, "zoo ob_dim %d outside [1, %d]: a policy-zoo MLP net reads the first ob_dim columns of the scene's observation", z->ob_dim, od);
  if (!(z->obs_clip > 0.0f)) FAIL(-9, "obs_clip %g must be positive", (double)z->obs_clip);
  r.zm.params = z->params; r.zm.filt = z->filt; r.zm.clip = z->obs_clip; r.zm.n = z->nzoo; r.zm.D = z->ob_dim;
  r.zm.L = make_layout(z->ob_dim, ad);
  return 0;
}
// (after the scratch is placed: the cell's rows -- embedding | previous latent | new latent, 64 floats each -- go behind the
// observation tile, 16-byte aligned, into the `rows_floats` floats the placed scratch holds there.  The table's state is agent 1's.)
static int place_zoo_lstm_table(RolloutArgs& r, const sumo_zoo_lstm* z, int od, int ad, int rows_floats) {
  if (!z->params || !z->filt) FAIL(-2, "sumo_zoo_lstm: missing buffer (params / filt)");
  if (!z->state) FAIL(-2, "sumo_zoo_lstm: missing state buffer (state)");
  if (z->nzoo < 1) FAIL(-7, "nzoo %d: the zoo table needs at least one entry", z->nzoo);
  if (z->ob_dim < 1 || z->ob_dim > od)
    FAIL(-4, "zoo ob_dim %d outside [1, %d]: a policy-zoo LSTM net reads the first ob_dim columns of the scene's observation", z->ob_dim, od);
  if (z->emb_dim != PT_H || z->hidden != 64) FAIL(-4, "zoo LSTM emb_dim %d / hidden %d: the fused launch is built for 64 / 64", z->emb_dim, z->hidden);
  if (!(z->obs_clip > 0.0f)) FAIL(-9, "obs_clip %g must be positive", (double)z->obs_clip);
  ZooLstmTable& q = r.zl;
  q.params = z->params; q.filt = z->filt; q.clip = z->obs_clip; q.forget_bias = z->forget_bias; q.n = z->nzoo; q.D = z->ob_dim; q.A = ad;
  q.emb = z->emb_dim;
  q.P = z->ob_dim * PT_H + PT_H + 2 * 64 * 256 + 256 + 64 * ad + 2 * ad;
  r.st1 = z->state;
  const int tile = 2 * r.XS;
  q.sc_off = tile;
  while ((2 * r.lds_off + q.sc_off) & 3) q.sc_off++;   // lds_off counts doubles from the 16-byte aligned LDS base
  if (q.sc_off + 3 * 64 > tile + rows_floats)
    FAIL(-8, "zoo LSTM scratch (observation tile + embedding and latent rows, %zu B) does not fit the policy scratch (%zu B)",
         (size_t)(q.sc_off + 3 * 64) * sizeof(float), (size_t)(tile + rows_floats) * sizeof(float));
  return 0;
}
// a league: the launch's checks of the struct (before the device is touched), then -- after the scratch is placed -- both tables
// and the entry of every tile
static int check_zoo_league(sumo_engine* E, const sumo_zoo_league* z, int npool, int env_offset) {
  if (z->mlp.nzoo < 1 || z->lstm.nzoo < 1)
    FAIL(-7, "sumo_zoo_league: nzoo %d (MLP table) / %d (LSTM table): a mixed league needs at least one net of each family (a league of one family plays through that family's launch)", z->mlp.nzoo, z->lstm.nzoo);
  if (npool != z->mlp.nzoo + z->lstm.nzoo) FAIL(-7, "npool %d must equal the league's size %d + %d", npool, z->mlp.nzoo, z->lstm.nzoo);
  if (z->tile_entry_dev && ((env_offset & 15) || (E->N & 15))) FAIL(-11, "a league entry per 16-env tile needs env_offset (%d) and the env count (%d) to be multiples of 16", env_offset, E->N);
  return 0;
}
static int place_zoo_league(RolloutArgs& r, const sumo_zoo_league* z, int od, int ad, int rows_floats) {
  if (int rc = place_zoo_mlp_table(r, &z->mlp, od, ad)) return rc;
  if (int rc = place_zoo_lstm_table(r, &z->lstm, od, ad, rows_floats)) return rc;
  r.tile_net = z->tile_entry_dev;
  return 0;
}

// ---- the seventeen entry points: env buffers, the family's checks (and the mode's), begin_*, the scratch of the learner's /
// checkpoints' side, the opponent table, launch.  Where a zoo MLP table comes before the scratch and a zoo LSTM table after it, that
// is the order in which the mode reports their errors. ----
extern "C" int sumo_rollout_steps(sumo_handle_t E, const sumo_rollout* ro, float* actions_dev, float* obs_dev, double* info_dev,
                                  uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, ro, b)) return rc;
  if (int rc = check_mlp_rollout(E, ro, NULL, false, &od, &ad)) return rc;
  if (ro->npool < 1) FAIL(-7, "npool %d", ro->npool);
  if (int rc = begin_mlp_rollout(E, ro, r)) return rc;
  if (int rc = place_mlp_scratch(E, ro->ob_dim, ro->ac_dim, r, 3)) return rc;
  return rollout_launch(E, r, 0, b, stream);
}

extern "C" int sumo_rollout_steps_lstm(sumo_handle_t E, const sumo_rollout_lstm* ro, float* actions_dev, float* obs_dev, double* info_dev,
                                       uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, ro, b)) return rc;
  if (int rc = check_lstm_rollout(E, ro, NULL, 0, &od, &ad)) return rc;
  if (int rc = begin_lstm_rollout(E, ro, od, 7, r)) return rc;   // zero row, previous latents [3], new latents [3]
  return rollout_launch(E, r, 1, b, stream);
}

extern "C" int sumo_rollout_steps_lstm_reuse(sumo_handle_t E, const sumo_rollout_lstm_reuse* rr, float* actions_dev, float* obs_dev, double* info_dev,
                                             uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, rr, b)) return rc;
  const sumo_rollout_lstm* ro = &rr->ro;
  if (!rr->state2) FAIL(-2, "sumo_rollout_lstm_reuse: missing buffer (state2)");
  if (int rc = check_lstm_rollout(E, ro, NULL, 0, &od, &ad)) return rc;
  if (int rc = begin_lstm_rollout(E, ro, od, 7, r)) return rc;   // the region of sumo_rollout_steps_lstm (one new latent row unused)
  r.st2 = rr->state2;
  return rollout_launch(E, r, 15, b, stream);
}

extern "C" int sumo_match_steps(sumo_handle_t E, const sumo_match* mo, float* actions_dev, float* obs_dev, double* info_dev,
                                uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, mo, b)) return rc;
  if (int rc = begin_mlp_match(E, mo, &od, &ad, r)) return rc;
  if (int rc = place_mlp_scratch(E, mo->ob_dim, mo->ac_dim, r, 2)) return rc;
  return rollout_launch(E, r, 2, b, stream);
}

extern "C" int sumo_match_steps_lstm(sumo_handle_t E, const sumo_match_lstm* mo, float* actions_dev, float* obs_dev, double* info_dev,
                                     uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, mo, b)) return rc;
  if (int rc = begin_lstm_match(E, mo, NULL, &od, &ad, r)) return rc;
  return rollout_launch(E, r, 3, b, stream);
}

extern "C" int sumo_rollout_steps_zoo(sumo_handle_t E, const sumo_rollout* ro, const sumo_zoo_mlp* z, float* actions_dev, float* obs_dev,
                                      double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, ro, b)) return rc;
  if (!z) FAIL(-1, "bad arguments");
  if (int rc = check_mlp_rollout(E, ro, "sumo_rollout_steps_zoo", false, &od, &ad)) return rc;
  if (ro->npool != z->nzoo) FAIL(-7, "npool %d must equal the zoo table's nzoo %d", ro->npool, z->nzoo);
  if (int rc = begin_mlp_rollout(E, ro, r)) return rc;
  if (int rc = place_zoo_mlp_table(r, z, od, ad)) return rc;
  if (int rc = place_mlp_scratch(E, ro->ob_dim, ro->ac_dim, r)) return rc;
  return rollout_launch(E, r, 4, b, stream);
}

extern "C" int sumo_match_steps_zoo(sumo_handle_t E, const sumo_match* mo, const sumo_zoo_mlp* z, float* actions_dev, float* obs_dev,
                                    double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, mo, b)) return rc;
  if (!z) FAIL(-1, "bad arguments");
  if (int rc = begin_mlp_match(E, mo, &od, &ad, r)) return rc;
  if (int rc = place_zoo_mlp_table(r, z, od, ad)) return rc;
  if (int rc = place_mlp_scratch(E, mo->ob_dim, mo->ac_dim, r)) return rc;
  return rollout_launch(E, r, 5, b, stream);
}

extern "C" int sumo_match_steps_zoo_lstm(sumo_handle_t E, const sumo_match* mo, const sumo_zoo_lstm* z, float* actions_dev, float* obs_dev,
                                         double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, mo, b)) return rc;
  if (!z) FAIL(-1, "bad arguments");
  if (int rc = begin_mlp_match(E, mo, &od, &ad, r)) return rc;
  if (int rc = place_mlp_scratch(E, mo->ob_dim, mo->ac_dim, r)) return rc;
  if (int rc = place_zoo_lstm_table(r, z, od, ad, 4 * PT_HS)) return rc;   // the two hidden tiles of agent 0's trunk
  return rollout_launch(E, r, 6, b, stream);
}

extern "C" int sumo_match_steps_lstm_zoo_lstm(sumo_handle_t E, const sumo_match_lstm* mo, const sumo_zoo_lstm* z, float* actions_dev,
                                              float* obs_dev, double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev,
                                              int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, mo, b)) return rc;
  if (!z) FAIL(-1, "bad arguments");
  if (int rc = begin_lstm_match(E, mo, "sumo_match_steps_lstm_zoo_lstm", &od, &ad, r)) return rc;
  if (int rc = place_zoo_lstm_table(r, z, od, ad, 2 * 128)) return rc;   // agent 0's previous and new latent
  return rollout_launch(E, r, 7, b, stream);
}

extern "C" int sumo_rollout_steps_zoo_lstm(sumo_handle_t E, const sumo_rollout* ro, const sumo_zoo_lstm* z, float* actions_dev, float* obs_dev,
                                           double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, ro, b)) return rc;
  if (!z) FAIL(-1, "bad arguments");
  if (int rc = check_mlp_rollout(E, ro, "sumo_rollout_steps_zoo_lstm", false, &od, &ad)) return rc;
  if (ro->npool != z->nzoo) FAIL(-7, "npool %d must equal the zoo table's nzoo %d", ro->npool, z->nzoo);
  if (int rc = begin_mlp_rollout(E, ro, r)) return rc;
  if (int rc = place_mlp_scratch(E, ro->ob_dim, ro->ac_dim, r)) return rc;
  if (int rc = place_zoo_lstm_table(r, z, od, ad, 4 * PT_HS)) return rc;   // the two hidden tiles of the learner's trunks
  return rollout_launch(E, r, 8, b, stream);
}

extern "C" int sumo_rollout_steps_lstm_zoo(sumo_handle_t E, const sumo_rollout_lstm* ro, const sumo_zoo_mlp* z, float* actions_dev, float* obs_dev,
                                           double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, ro, b)) return rc;
  if (!z) FAIL(-1, "bad arguments");
  if (int rc = check_lstm_rollout(E, ro, "sumo_rollout_steps_lstm_zoo", z->nzoo, &od, &ad)) return rc;
  if (int rc = place_zoo_mlp_table(r, z, od, ad)) return rc;                      // (needs no scratch: its errors come first)
  if (int rc = begin_lstm_rollout(E, ro, od, LSTM_ZOO_ROWS, r)) return rc;
  return rollout_launch(E, r, 9, b, stream);
}

extern "C" int sumo_rollout_steps_lstm_zoo_lstm(sumo_handle_t E, const sumo_rollout_lstm* ro, const sumo_zoo_lstm* z, float* actions_dev,
                                                float* obs_dev, double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev,
                                                int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, ro, b)) return rc;
  if (!z) FAIL(-1, "bad arguments");
  if (int rc = check_lstm_rollout(E, ro, "sumo_rollout_steps_lstm_zoo_lstm", z->nzoo, &od, &ad)) return rc;
  if (int rc = begin_lstm_rollout(E, ro, od, LSTM_ZOO_ROWS, r)) return rc;
  if (int rc = place_zoo_lstm_table(r, z, od, ad, LSTM_ZOO_ROWS * 128)) return rc;   // the cell's rows go where the learner's latent rows were
  return rollout_launch(E, r, 10, b, stream);
}

extern "C" int sumo_rollout_steps_zoo_league(sumo_handle_t E, const sumo_rollout* ro, const sumo_zoo_league* z, float* actions_dev, float* obs_dev,
                                             double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, ro, b)) return rc;
  if (!z) FAIL(-1, "bad arguments");
  if (int rc = check_mlp_rollout(E, ro, "sumo_rollout_steps_zoo_league", true, &od, &ad)) return rc;
  if (int rc = check_zoo_league(E, z, ro->npool, ro->env_offset)) return rc;
  if (int rc = begin_mlp_rollout(E, ro, r)) return rc;
  if (int rc = place_mlp_scratch(E, ro->ob_dim, ro->ac_dim, r)) return rc;   // the zoo trunk's hidden tiles are the learner's ...
  if (int rc = place_zoo_league(r, z, od, ad, 4 * PT_HS)) return rc;         // ... and the cell's rows go there too, as in mode 8
  return rollout_launch(E, r, 11, b, stream);
}

extern "C" int sumo_rollout_steps_lstm_zoo_league(sumo_handle_t E, const sumo_rollout_lstm* ro, const sumo_zoo_league* z, float* actions_dev,
                                                  float* obs_dev, double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev,
                                                  int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, ro, b)) return rc;
  if (!z) FAIL(-1, "bad arguments");
  if (ro->tile_net_dev) FAIL(-2, "sumo_rollout_steps_lstm_zoo_league: tile_net_dev must be NULL (the league's tile_entry_dev selects the nets)");
  if (int rc = check_lstm_rollout(E, ro, "sumo_rollout_steps_lstm_zoo_league", z->mlp.nzoo + z->lstm.nzoo, &od, &ad)) return rc;
  if (int rc = check_zoo_league(E, z, ro->npool, ro->env_offset)) return rc;
  if (int rc = begin_lstm_rollout(E, ro, od, LSTM_ZOO_ROWS, r)) return rc;   // the rows hold the larger of the two zoo passes (static_assert above)
  if (int rc = place_zoo_league(r, z, od, ad, LSTM_ZOO_ROWS * 128)) return rc;
  return rollout_launch(E, r, 12, b, stream);
}

extern "C" int sumo_match_steps_cross(sumo_handle_t E, const sumo_match_cross* mo, float* actions_dev, float* obs_dev, double* info_dev,
                                      uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, mo, b)) return rc;
  if (mo->lstm_side != 0 && mo->lstm_side != 1) FAIL(-9, "lstm_side %d: 0 (agent 0 plays the LSTM checkpoints) or 1", mo->lstm_side);
  // each family's half of the struct goes through that family's checks: the one state buffer stands for both of sumo_match_lstm's
  const sumo_match_lstm ml = {mo->proto, mo->nets_dev, mo->idx0, mo->idx1, mo->nsnap_lstm, mo->state, mo->state,
                              mo->T, mo->s0, mo->K, mo->quota, mo->noise0, mo->noise1, mo->score};
  const sumo_match mm = {mo->params, mo->idx0, mo->idx1, mo->nsnap_mlp, mo->ob_dim, mo->ac_dim,
                         mo->T, mo->s0, mo->K, mo->quota, mo->noise0, mo->noise1, mo->score};
  if (int rc = begin_lstm_match(E, &ml, NULL, &od, &ad, r, LSTM_MLP_MATCH_ROWS)) return rc;
  r.nsnap_lstm = r.nsnap; r.lstm_side = mo->lstm_side;
  if (int rc = begin_mlp_match(E, &mm, &od, &ad, r)) return rc;   // (leaves nsnap at the MLP table's size)
  r.L = make_layout(mo->ob_dim, mo->ac_dim);
  return rollout_launch(E, r, 13, b, stream);
}

extern "C" int sumo_match_steps_lstm_zoo(sumo_handle_t E, const sumo_match_lstm* mo, const sumo_zoo_mlp* z, float* actions_dev, float* obs_dev,
                                         double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  int od = 0, ad = 0;
  if (int rc = check_launch_args(E, mo, b)) return rc;
  if (!z) FAIL(-1, "bad arguments");
  if (int rc = begin_lstm_match(E, mo, "sumo_match_steps_lstm_zoo", &od, &ad, r, LSTM_MLP_MATCH_ROWS)) return rc;
  if (int rc = place_zoo_mlp_table(r, z, od, ad)) return rc;
  return rollout_launch(E, r, 14, b, stream);
}

// Co-training on a match-up of two species (mode 16).  The entry has its own scene check: rollout_scene keeps refusing mixed scenes for
// the other entries, here each side is held against ITS agent of the scene (a homogeneous scene is simply a valid one).
static int check_pair_rollout(sumo_engine* E, const sumo_rollout_pair* ro) {
  const sumo_model_t* m = &E->hm;
  if (E->cfrc_mode) FAIL(-12, "cfrc_mode rne_post fills the observations in a second launch per step: use sumo_step (the fused rollout evaluates the policies inside its launch)");
  if (ro->T < 1 || ro->K < 1 || ro->s0 < 0 || ro->s0 + ro->K > ro->T) FAIL(-5, "steps [%d, %d) outside the rollout buffers (T = %d)", ro->s0, ro->s0 + ro->K, ro->T);
  if (ro->env_offset < 0 || ro->env_offset + E->N > ro->Ntot) FAIL(-6, "envs [%d, %d) outside the rollout buffers (N = %d)", ro->env_offset, ro->env_offset + E->N, ro->Ntot);
  const int* anq = SUMO_I(m, agent_nq); const int* anv = SUMO_I(m, agent_nv); const int* anb = SUMO_I(m, agent_nbody);
  const int* anu = SUMO_I(m, agent_nu);
  for (int g = 0; g < 2; g++) {
    const sumo_pair_side& p = ro->side[g];
    const int od = anq[g] + anv[g] + 6 * anb[g] + 14, ad = anu[g];
    if (p.ob_dim != od || p.ac_dim != ad) FAIL(-4, "side %d: ob_dim %d / ac_dim %d do not match agent %d of the scene (%d / %d)", g, p.ob_dim, p.ac_dim, g, od, ad);
    if (p.ac_dim > PT_MAXA) FAIL(-16, "side %d: ac_dim %d above the %d columns of a head", g, p.ac_dim, PT_MAXA);
    if (p.nrows < 1) FAIL(-7, "side %d: nrows %d: the table needs at least one row", g, p.nrows);
    const int P = make_layout(p.ob_dim, p.ac_dim).P;
    if (p.row_stride < P) FAIL(-17, "side %d: row_stride %d below the %d parameters of a row", g, p.row_stride, P);
    if (!p.table) FAIL(-13, "side %d: missing parameter table", g);
    if (!p.noise) FAIL(-14, "side %d: missing noise", g);
    if (!p.obs || !p.act || !p.val || !p.nlp || !p.done) FAIL(-15, "side %d: missing record buffer (obs / act / val / nlp / done)", g);
    if (p.tile_row && ((ro->env_offset & 15) || (E->N & 15)))
      FAIL(-11, "side %d: a table row per 16-env tile needs env_offset (%d) and the env count (%d) to be multiples of 16", g, ro->env_offset, E->N);
  }
  if (!ro->rew || !ro->ep_done || !ro->ep_r || !ro->ep_l) FAIL(-2, "sumo_rollout_pair: missing buffer (rew / ep_done / ep_r / ep_l)");
  return 0;
}

extern "C" int sumo_rollout_steps_pair(sumo_handle_t E, const sumo_rollout_pair* ro, float* actions_dev, float* obs_dev, double* info_dev,
                                       uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream) {
  const EnvBuffers b = {actions_dev, obs_dev, info_dev, done_dev, ep_r_dev, ep_dr_dev, ep_l_dev};
  RolloutArgs r = {};
  if (int rc = check_launch_args(E, ro, b)) return rc;
  if (int rc = check_pair_rollout(E, ro)) return rc;
  HIPCHK(hipSetDevice(E->device));
  for (int g = 0; g < 2; g++) {
    const sumo_pair_side& p = ro->side[g];
    PairSideArgs& q = r.pair[g];
    q.table = p.table; q.tile_row = p.tile_row; q.obs = p.obs; q.act = p.act; q.val = p.val; q.nlp = p.nlp; q.done = p.done;
    q.nrows = p.nrows; q.row_stride = p.row_stride; q.record_row = p.record_row; q.L = make_layout(p.ob_dim, p.ac_dim);
  }
  r.noise0 = ro->side[0].noise; r.noise1 = ro->side[1].noise;
  r.rew = ro->rew; r.ep_done = ro->ep_done; r.ep_r = ro->ep_r; r.ep_l = ro->ep_l; r.alpha = ro->alpha;
  r.T = ro->T; r.Ntot = ro->Ntot; r.env_offset = ro->env_offset; r.s0 = ro->s0; r.K = ro->K;
  // x [2][XS], XS the wider side's padded width, and one pass's activation rows [2][PT_VS] (policy and value trunk of a recording side)
  const int dmax = ro->side[0].ob_dim > ro->side[1].ob_dim ? ro->side[0].ob_dim : ro->side[1].ob_dim;
  const int amax = ro->side[0].ac_dim > ro->side[1].ac_dim ? ro->side[0].ac_dim : ro->side[1].ac_dim;
  if (int rc = place_mlp_scratch(E, dmax, amax, r, 1)) return rc;
  return rollout_launch(E, r, 16, b, stream);
}
