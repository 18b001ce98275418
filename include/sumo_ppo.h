/* sumo_ppo.h -- C ABI of the MI355X-native PPO2 self-play arithmetic (libsumo_ppo.so).
 *
 * Stands in for the TF1 graph + numpy glue of the reference's learner/rollout path.  Each entry point names the
 * reference code it replaces (paths relative to the reference checkout):
 *
 *   ppo_param_count / layout    PPOModel.save/load variable order (model.py:153-177):
 *                               pi/mlp_fc0/{w,b} pi/mlp_fc1/{w,b} vf/mlp_fc0/{w,b} vf/mlp_fc1/{w,b} pi/{w,b,logstd} vf/{w,b}
 *                               flattened row-major into ONE float32 vector, w stored [in][out] as TF does.
 *   ppo_forward                 PolicyWithValue.step / .value / .action_probability (policies.py:84-128) over the
 *                               mlp(64,64,relu) trunks (baselines/baselines/common/models.py:74-103) and the diagonal
 *                               Gaussian head (baselines/baselines/common/distributions.py:96-113,227-251)
 *   ppo_reward_mix              Runner.run reward curriculum (runner.py:127-143)
 *   ppo_vtrace                  Runner.run IS ratios + V-trace targets (runner.py:166-196)
 *   ppo_adv_moments/_normalize  PPOModel.train advantage normalisation (model.py:180-185); split in two so a
 *                               multi-GPU run can all-reduce the three moments in between
 *   ppo_selection_scores        the 'ours' opponent selector's candidate scores (alg_ppo.py:227-244), all candidates in one launch
 *   ppo_grad                    loss + gradients of model.py:65-132 (sums, not means: divide by the global count)
 *   ppo_a2c_grad / _loss_stats  loss + gradients and statistics of ActorCriticModel (model.py:257-310)
 *   ppo_clip_adam               tf.clip_by_global_norm + tf.train.AdamOptimizer(epsilon=1e-5).apply_gradients
 *                               (model.py:121-139)
 *
 * All pointers are DEVICE pointers owned by the caller; `stream` is a hipStream_t as void*.  Return 0 / negative
 * + ppo_last_error().  float32 arithmetic on MFMA (v_mfma_f32_16x16x4_f32, exact f32) for the dense layers.
 */
#ifndef SUMO_PPO_H
#define SUMO_PPO_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPO_HIDDEN 64
#define PPO_NSTATS 8 /* sum pg, sum vf, entropy, sum approxkl, sum clipfrac, sum w (unused), count, grad norm */

const char* ppo_last_error(void);
int ppo_param_count(int ob_dim, int ac_dim);

/* flags for ppo_forward */
#define PPO_FWD_PI 1        /* evaluate the policy trunk: mean / action / neglogp */
#define PPO_FWD_VF 2        /* evaluate the value trunk: value */
/* obs [n][obs_stride]; noise, given_action, action_out, mean_out [n][ac_dim] (any may be NULL);
 * action = given_action if given, else mean + exp(logstd)*noise if noise given, else mean (deterministic);
 * neglogp_out [n] = -log pi(action | obs); value_out [n]. */
int ppo_forward(const float* params, const float* obs, int n, int obs_stride, int ob_dim, int ac_dim, int flags,
                const float* noise, const float* given_action, float* action_out, float* neglogp_out,
                float* value_out, float* mean_out, void* stream);
/* Same, for the fixed opponents of the policy zoo (robosumo/robosumo/policy_zoo/policy.py:23-91, utils.py:9-33): tanh
 * hidden units (flag PPO_FWD_TANH) and the running-mean observation filter clip((obs - mean) * invstd, -clip, clip)
 * applied to the ob_dim columns read (obs_mean / obs_invstd float32 [ob_dim]; both NULL = no filter). */
#define PPO_FWD_TANH 4
int ppo_forward_filtered(const float* params, const float* obs, int n, int obs_stride, int ob_dim, int ac_dim, int flags,
                         const float* obs_mean, const float* obs_invstd, float obs_clip, const float* noise,
                         const float* given_action, float* action_out, float* neglogp_out, float* value_out,
                         float* mean_out, void* stream);

/* One time step of an LSTM policy for n rows (envs), state carried by the caller.  Covers the two recurrent nets of the
 * reference tree:
 *   - baselines `lstm(nlstm)` (baselines/baselines/common/models.py:131-183 + a2c/utils.py:82-103): x = obs, gates
 *     z = x*wx + h*wh + b split as (i, f, o, u), c,h first multiplied by (1 - mask), shared latent for both heads
 *     (policies.py:160-181);  gate_order = PPO_LSTM_GATES_IFOU, forget_bias = 0
 *   - policy-zoo `LSTMPolicy` (robosumo/robosumo/policy_zoo/policy.py:94-199): observation filter, one relu embedding
 *     layer, tf BasicLSTMCell (kernel [x|h] -> (i, j, f, o), forget bias 1);  gate_order = PPO_LSTM_GATES_IJFO
 * All weights are [in][out] row-major float32 device pointers.  emb_w == NULL: no embedding (x = filtered obs).
 * wh points at the recurrent rows (for a TF kernel: kernel + x_dim * 4 * hidden).  c / h are read and overwritten
 * ([n] rows of `state_stride` floats each); mask float32 [n] or NULL.  Heads (each optional): head_w [hidden][ac_dim],
 * head_b, logstd -> mean / action / neglogp exactly as ppo_forward; vf_w [hidden], vf_b -> value_out. */
#define PPO_LSTM_GATES_IFOU 0
#define PPO_LSTM_GATES_IJFO 1
typedef struct ppo_lstm_net {
  int ob_dim, emb_dim, hidden, ac_dim, gate_order;
  float forget_bias;
  const float *obs_mean, *obs_invstd; float obs_clip;     /* optional observation filter (both NULL = none) */
  const float *emb_w, *emb_b;                             /* optional embedding [ob_dim][emb_dim] + relu */
  const float *wx, *wh, *b;                               /* [x_dim][4*hidden], [hidden][4*hidden], [4*hidden] */
  const float *head_w, *head_b, *logstd;                  /* optional Gaussian head */
  const float *vf_w, *vf_b;                               /* optional value head */
} ppo_lstm_net;
int ppo_lstm_step(const ppo_lstm_net* net, const float* obs, int n, int obs_stride, const float* mask, float* c, float* h,
                  int state_stride, const float* noise, const float* given_action, float* action_out, float* neglogp_out,
                  float* value_out, float* mean_out, void* stream);

/* ppo_lstm_step against a POOL of frozen nets (BASELINE config 5: 16 opponent snapshots, one per env tile; the reference loads one
 * snapshot for all envs per update, alg_ppo.py:213-214): rows 16 t .. 16 t + 15 are evaluated with nets_dev[tile_net_dev[t]].
 * `proto` (host) gives the dimensions / gate order every net of the pool shares and is checked like ppo_lstm_step's net;
 * nets_dev is a DEVICE array of ppo_lstm_net whose pointers address each snapshot's weights, tile_net_dev DEVICE int32
 * [ceil(n / 16)].  Everything else as ppo_lstm_step (one launch for all tiles). */
int ppo_lstm_step_pool(const ppo_lstm_net* proto, const ppo_lstm_net* nets_dev, const int32_t* tile_net_dev, const float* obs, int n,
                       int obs_stride, const float* mask, float* c, float* h, int state_stride, const float* noise,
                       const float* given_action, float* action_out, float* neglogp_out, float* value_out, float* mean_out,
                       void* stream);

/* One seat of a zoo-vs-zoo match: the actions of one agent of n envs in ONE launch, every 16-env tile played by its own policy-zoo
 * net, MLP nets and LSTM(64) nets mixed (robosumo/demos/play.py puts one zoo net on each side of any of the nine scenes).
 *   obs          row e at obs + e * obs_stride (the seat's slice of the env's observation buffer); ob_dim columns are read
 *   done         the previous step's flag of env e at done[e * done_stride] (uint8; NULL = none): an LSTM tile's state rows are
 *                zeroed where it is set, before the cell runs; MLP tiles do not touch `state`
 *   noise        contiguous [n][ac_dim] standard-normal rows; NULL = the action is the mean
 *   action_out   row e at action_out + e * act_stride (the seat's slice of the env's action buffer); ac_dim columns are written
 * An MLP tile yields the bits of ppo_forward_filtered(flags = PPO_FWD_PI | PPO_FWD_TANH, that row's filter, noise) on its 16 rows, an
 * LSTM tile the actions and the new state of ppo_lstm_step with that row's net (PPO_LSTM_GATES_IJFO, embedding and hidden 64): the
 * kernels share one copy of each body.  A tile whose entry is outside [0, n_mlp + n_lstm) writes neither actions nor state and reads
 * no table; 1 + tile is stored to status_dev (DEVICE int32, may be NULL; the caller zeroes it).  Argument errors (NULL seat / obs /
 * action_out / tile_entry, n < 16 or off the tile grid, ob_dim outside [1, 512], ac_dim outside [1, 16], strides below the widths,
 * no rows, rows without a table, LSTM rows without a state) return before anything is launched. */
typedef struct ppo_zoo_seat {
  const float *mlp_params, *mlp_filt;    /* [n_mlp][Pm] in policy_zoo.zoo_kernel_flat order; [n_mlp][2][ob_dim] mean | 1/std */
  const float *lstm_params, *lstm_filt;  /* [n_lstm][Pl] in policy_zoo._ZOO_LSTM_ROW order; [n_lstm][2][ob_dim] */
  const int32_t* tile_entry;             /* DEVICE [n / 16]: e < n_mlp -> MLP row e; n_mlp <= e < n_mlp + n_lstm -> LSTM row e - n_mlp
                                            (the encoding of policy_zoo.league_entries) */
  float* state;                          /* DEVICE [n][128] c | h of the LSTM tiles; NULL allowed only when n_lstm == 0 */
  int n_mlp, n_lstm, ob_dim, ac_dim;
  float obs_clip, forget_bias;
} ppo_zoo_seat;
int ppo_zoo_seat_act(const ppo_zoo_seat* seat, const float* obs, int n, int obs_stride, const uint8_t* done, int done_stride,
                     const float* noise, float* action_out, int act_stride, int32_t* status_dev, void* stream);

/* One step of a MIXED match-up (RoboSumo-Ant-vs-Bug-v0, ...: the two sides differ in observation and action width) for both seats in
 * ONE launch, grid (n / 16 tiles, 2 sides): agent 0 is played by a learner's MLP(64,64) net, agent 1 by a zoo seat.
 *   side 0  tile t is evaluated with row tile_row[t] (NULL = row 0 for every tile) of `table`, nrows rows of row_stride floats, each an
 *           MLP(64,64) + copy-value parameter vector in ppo_forward's flat order (ppo_param_count(ob_dim, ac_dim) floats).  obs0 row e at
 *           obs0 + e * obs_stride, action0 row e at action0 + e * act_stride (ac_dim columns written), noise0 contiguous [n][ac_dim] or
 *           NULL (= the action is the mean).  Action, neglogp and value are the bits of ppo_forward(row, obs0, PPO_FWD_PI | PPO_FWD_VF,
 *           noise0).  `record` (NULL or any member NULL = skip it) receives the step's rollout record: obs [n][ob_dim] an exact copy of
 *           the rows read, action [n][ac_dim], neglogp [n], value [n] and done [n] = done[e * done_stride], agent 0's flag of the
 *           previous step.  With record->value NULL the value trunk is not evaluated.
 *   side 1  ppo_zoo_seat_act(seat, obs1, ..., noise1, action1, ...) bit for bit, the same device function: an LSTM tile's state rows
 *           are reset on done[e * done_stride] -- agent 0's flag, the one side 0 records.
 * n, the strides and `done` are shared by the two sides (the env's buffers).  A tile whose learner row is outside [0, nrows), or whose
 * zoo entry names no net, reads no table and writes neither actions, record nor state for that side; it stores
 *   status = 1 + 2 * tile + side            (tile = (status - 1) >> 1, side = (status - 1) & 1)
 * to status_dev (DEVICE int32, may be NULL; the caller zeroes it; of several such tiles one is reported).  Argument errors return
 * before anything is launched: NULL learner / table / obs0 / action0, nrows < 1, learner ob_dim outside [1, 512] or ac_dim outside
 * [1, 16], strides below the learner's widths, row_stride below the parameter count, and everything ppo_zoo_seat_act refuses of its
 * seat, n and strides. */
typedef struct ppo_learner_seat {
  const float* table;        /* DEVICE [nrows][row_stride] */
  const int32_t* tile_row;   /* DEVICE [n / 16], or NULL: row 0 for every tile */
  int nrows, row_stride, ob_dim, ac_dim;
} ppo_learner_seat;
typedef struct ppo_mixed_record {
  float *obs, *action, *neglogp, *value;
  uint8_t* done;
} ppo_mixed_record;
int ppo_mixed_step(const ppo_learner_seat* learner, const ppo_zoo_seat* seat, const float* obs0, const float* obs1, int n,
                   int obs_stride, const uint8_t* done, int done_stride, const float* noise0, const float* noise1, float* action0,
                   float* action1, int act_stride, const ppo_mixed_record* record, int32_t* status_dev, void* stream);

/* One step of a mixed match-up with a LEARNER seat on BOTH sides (two species trained against each other), ONE launch, grid (n / 16
 * tiles, 2 sides).  Each side is side 0 of ppo_mixed_step, the same device function, with its own widths, table, buffers and record:
 * per side, action, neglogp and value are the bits of ppo_forward(row, obs, PPO_FWD_PI | PPO_FWD_VF, noise), the obs record is an exact
 * copy of the rows read and the done record is that side's own flag done[e * done_stride] (NULL = 0).  n and the three strides are
 * shared (the env's buffers).  A tile whose row is outside [0, nrows) reads no table and writes nothing for that side; it stores
 * status = 1 + 2 * tile + side to status_dev (DEVICE int32, may be NULL; the caller zeroes it), the encoding of ppo_mixed_step.
 * Argument errors return before anything is launched, the message naming the side: NULL sides / table / obs / action, nrows < 1,
 * ob_dim outside [1, 512] or ac_dim outside [1, 16], strides below a side's widths, row_stride below the parameter count, n < 16 or
 * off the 16 grid, done given with done_stride < 1. */
typedef struct ppo_pair_side {
  ppo_learner_seat seat;      /* table, tile_row (NULL = row 0), nrows, row_stride, ob_dim, ac_dim */
  const float *obs, *noise;   /* obs row e at obs + e*obs_stride; noise contiguous [n][ac_dim] or NULL = means */
  const uint8_t* done;        /* this agent's previous-step flag at done[e*done_stride]; NULL = 0 */
  float* action;              /* row e at action + e*act_stride */
  ppo_mixed_record record;    /* any member NULL = skip; value NULL = value trunk not evaluated */
} ppo_pair_side;
int ppo_mixed_pair_step(const ppo_pair_side sides[2], int n, int obs_stride, int done_stride, int act_stride,
                        int32_t* status_dev, void* stream);

/* --- recurrent training (back-propagation through time over the baselines LSTM; the reference builds the unrolled graph in
 * a2c/utils.py:82-103 + model.py:65-139, its own recurrent minibatch loop alg_ppo.py:408-421 is dead code) ---------------
 * ppo_lstm_step_save: ppo_lstm_step that also records what the backward pass needs for this time step:
 *   save_gates [n][4*hidden] activated gates in the net's column order, save_cprev / save_hprev [n][hidden] the masked
 *   previous state, save_tanhc [n][hidden] tanh of the new cell state (the new h is the latent: read it from `h`). */
int ppo_lstm_step_save(const ppo_lstm_net* net, const float* obs, int n, int obs_stride, const float* mask, float* c, float* h,
                       int state_stride, float* save_gates, float* save_cprev, float* save_hprev, float* save_tanhc, void* stream);
/* The unrolled forward with the input block hoisted out of the recurrence: ppo_lstm_xproj computes z_out [rows][4*hidden] = x * wx
 * for all rows = (time, env) pairs of a minibatch in one launch (same tiles and k order as the step kernel's input block);
 * ppo_lstm_step_save_z is ppo_lstm_step_save for one time step whose gate sums start from z_t [n][4*hidden] (that step's rows of
 * z_out) instead of from the observations -- bit-identical to ppo_lstm_step_save on the same inputs, with half the dependent
 * chain per step -- and also writes the new latent to latent_out [n][hidden] (NULL = skip).  Nets without embedding /
 * observation filter only (what learn(network='lstm') trains). */
int ppo_lstm_xproj(const ppo_lstm_net* net, const float* obs, int rows, int obs_stride, float* z_out, void* stream);
int ppo_lstm_step_save_z(const ppo_lstm_net* net, const float* z_t, int n, const float* mask, float* c, float* h, int state_stride,
                         float* save_gates, float* save_cprev, float* save_hprev, float* save_tanhc, float* latent_out, void* stream);
/* All T steps in one launch each (hidden 128, gate order i,f,o,u): a workgroup of eight waves owns a 16-row tile of env sequences for
 * the whole sequence and keeps its slice of wh in registers; time-major buffers [T][n][...], mask [T][n] (NULL = none).
 *   ppo_lstm_seq_forward   z0 = ppo_lstm_xproj of all rows; c / h [n] (state_stride) hold the state at the start and receive the state
 *                          after step T-1; records as ppo_lstm_step_save per step + latent [T][n][128].  Same numbers as T calls of
 *                          ppo_lstm_step_save_z, bit for bit.
 *   ppo_lstm_seq_backward  BPTT from zero carries: dz_out [T][n][512] as T calls of ppo_lstm_bwd_step from t = T-1 down (the
 *                          contraction dz * wh^T is summed in one chain instead of four partial tiles: equal up to rounding). */
int ppo_lstm_seq_forward(const ppo_lstm_net* net, const float* z0, int T, int n, const float* mask, float* c, float* h, int state_stride,
                         float* save_gates, float* save_cprev, float* save_hprev, float* save_tanhc, float* latent, void* stream);
int ppo_lstm_seq_backward(const ppo_lstm_net* net, int T, int n, const float* dlatent, const float* mask, const float* gates,
                          const float* cprev, const float* tanhc, float* dz_out, void* stream);
/* PPO loss heads on stored latents (rows = all (time, env) pairs of the minibatch): forward of the Gaussian / value heads,
 * loss terms of model.py:65-111 and their gradients.  Outputs: dlatent [rows][hidden], dmean [rows][ac_dim], dvalue [rows],
 * dlogstd_rows [rows][ac_dim] (sum over rows - ent_coef = d loss / d logstd), stats double[PPO_NSTATS] (+= un-normalised sums
 * as ppo_grad; stats[2] is not touched).  inv_count = 1 / (global number of rows).  A row whose old neglogp is NaN gets ratio 2 and
 * zero dmean / dlogstd_rows (model.py:96) and is counted in stats[4], but its nlp - old still enters stats[3]: stats[3] is left NaN, as
 * the reference's approxkl is. */
int ppo_lstm_head_grad(const ppo_lstm_net* net, const float* latent, int rows, const float* actions, const float* adv,
                       const float* returns, const float* old_neglogp, const float* is_weight, double inv_count, float cliprange,
                       float vf_coef, float* dlatent, float* dmean, float* dvalue, float* dlogstd_rows, double* stats, void* stream);
/* ppo_lstm_head_grad with a ROW MASK (opponent-data reuse for recurrent learners: an unusable row cannot be cut out of a sequence,
 * it stays in the recurrence and leaves the loss).  valid float32 [rows] holds 0 or 1.  A row with valid = 0 writes exact zeros to
 * dlatent, dmean, dvalue and dlogstd_rows and adds nothing to any stats entry (stats[6] counts valid rows only; a NaN on such a row
 * reaches nothing); a valid row runs the arithmetic of ppo_lstm_head_grad unchanged (the value term stays unweighted by is_weight).
 * inv_count = (float)(1 / max(*count_dev, 1)) is read on the DEVICE (count_dev: the third moment of ppo_adv_moments_masked_ws), so a
 * captured graph replays with another number of valid rows. */
int ppo_lstm_head_grad_masked(const ppo_lstm_net* net, const float* latent, int rows, const float* actions, const float* adv,
                              const float* returns, const float* old_neglogp, const float* is_weight, const float* valid,
                              const double* count_dev, float cliprange, float vf_coef, float* dlatent, float* dmean, float* dvalue,
                              float* dlogstd_rows, double* stats, void* stream);
/* One step of BPTT (gate order i,f,o,u): dh_carry / dc_carry [n][hidden] hold d loss / d (h_t, c_t) flowing from later steps and
 * are replaced by the values for step t-1 (already multiplied by 1 - mask_t); dz_out [n][4*hidden] receives d loss / d
 * (pre-activation gates), whose products with the inputs give the weight gradients (plain GEMMs, done by the caller).
 * net->wh is read with 16-byte vector loads: it must be 16-byte aligned (the model's flat parameter layout guarantees it). */
int ppo_lstm_bwd_step(const ppo_lstm_net* net, int n, const float* dlatent_t, const float* mask_t, const float* gates_t,
                      const float* cprev_t, const float* tanhc_t, float* dh_carry, float* dc_carry, float* dz_out, void* stream);

/* Weight gradients of the recurrent PPO step from the stored forward records and the deltas of the backward sweep (the matmuls
 * TF's autodiff emits for a2c/utils.py:82-103 + the heads of policies.py:50,70): over all `rows` = (time, env) pairs,
 *   [x | h_prev | 1]^T dz -> wx, wh, b      and      [latent | 1]^T [dmean | dvalue | dlogstd_rows] -> pi/w, pi/b, logstd, vf/w, vf/b
 * written into `grads` in checkpoint order (wx | wh | b | pi/w | pi/b | logstd | vf/w | vf/b); logstd_shift is added to the
 * logstd gradient (the entropy term - ent_coef / world).  x [rows][ob_dim], hprev / latent [rows][hidden], dz [rows][4 hidden],
 * dmean / dlogstd_rows [rows][ac_dim], dvalue [rows].  Split-K MFMA kernel + fixed-order slab reduction (deterministic).
 * workspace: ppo_lstm_wgrad_workspace_bytes(ob_dim, hidden, ac_dim) bytes, sized for hidden 64 / 128, ob_dim 1..512, ac_dim 1..16:
 * anything else is an argument error (negative code, nothing launched). */
size_t ppo_lstm_wgrad_workspace_bytes(int ob_dim, int hidden, int ac_dim);
int ppo_lstm_wgrad(const ppo_lstm_net* net, int rows, const float* x, const float* hprev, const float* dz, const float* latent,
                   const float* dmean, const float* dvalue, const float* dlogstd_rows, float logstd_shift, float* grads, void* workspace,
                   void* stream);

/* info float64 [n][2][8] as written by sumo_step (slot 6 shaping, slot 3 main); reward_out float32 [2][n]
 * (agent-major, one time slice of the rollout buffer) = alpha*shaping + (1-alpha)*main evaluated in float64. */
int ppo_reward_mix(const double* info, int n, double alpha, float* reward_out, int agent_stride, void* stream);

/* ppo_reward_mix plus the step's episode records (agent 0's done flag, episode return and length as the monitor wrapper
 * reports them, bench/monitor.py:63-78) copied into one time slice of the rollout buffers: one launch per rollout step.
 * done uint8 [n][2]; ep_r float64 [n]; ep_l int32 [n]. */
int ppo_post_step(const double* info, int n, double alpha, float* reward_out, int agent_stride, const uint8_t* done,
                  const double* ep_r, const int32_t* ep_l, uint8_t* ep_done_out, double* ep_r_out, int32_t* ep_l_out, void* stream);

/* The five policy/value evaluations of one self-play rollout step (runner.py:62-96) in one launch, relu MLP nets.
 * obs: observation of env e, agent g at obs + e*env_stride + g*agent_stride (float32, ob_dim values); the learner acts on
 * agent 0 and the opponent on agent 1 (action = mean + exp(logstd) * noise_g[e]), each action is scored by the other net,
 * and the learner's value net is evaluated on both agents' observations.
 * act_env float32 [n][2][ac_dim] receives both actions (the env's action buffer).
 * out_f32[10] = { obs_out0, obs_out1 (float32 [n][ob_dim] copies of the inputs, may be NULL), act0, act1 ([n][ac_dim]),
 *                 nlp0, nlp1 (learner's neglogp of the action on side g), onlp0, onlp1 (opponent's), val0, val1 ([n]) }.
 * out_done (may be NULL) = { done_out0, done_out1 } uint8 [n] copies of done_in[e][g] (done_in uint8 [n][2], may be NULL).
 * Outputs equal those of the corresponding four ppo_forward calls bit for bit. */
int ppo_selfplay_forward(const float* learner_params, const float* opponent_params, const float* obs, int n, int env_stride,
                         int agent_stride, int ob_dim, int ac_dim, const float* noise0, const float* noise1,
                         const uint8_t* done_in, float* act_env, float* const* out_f32, uint8_t* const* out_done, void* stream);

/* Buffers [2][T][N] float32 (agent, time, env); dones uint8 [2][T][N] = done flags BEFORE each step; last_dones uint8
 * [N][2]; last_values float32 [2][N].  Outputs returns float32 [2][T][N], ratios float32 [T][N]. */
int ppo_vtrace(const float* rewards, const float* values, const float* neglogp, const float* opp_neglogp,
               const uint8_t* dones, const uint8_t* last_dones, const float* last_values, int T, int N, double gamma,
               double lam, double rho_bar, double c_bar, float* returns, float* off_policy_ratio, float* off_env_ratio,
               float* ratio, void* stream);

/* minibatch rows are data rows idx[0..n) (idx may be NULL = identity).  moments double[3] = {sum adv, sum adv^2, n}
 * with adv = returns - values.  Deterministic (fixed summation order), any n.  ppo_adv_moments_ws keeps its per-block partial sums
 * and arrival counter in the caller's workspace (ppo_adv_moments_workspace_bytes() bytes, zero-initialised once; one call in flight per
 * workspace): models stepping concurrently on different streams do not share state.  ppo_adv_moments is the convenience form on
 * library-owned workspaces handed out round robin (16; one device per process). */
size_t ppo_adv_moments_workspace_bytes(void);
int ppo_adv_moments_ws(const float* returns, const float* values, const int32_t* idx, int n, double* moments, void* workspace, void* stream);
int ppo_adv_moments(const float* returns, const float* values, const int32_t* idx, int n, double* moments, void* stream);
int ppo_adv_normalize(const float* returns, const float* values, const int32_t* idx, int n, const double* moments,
                      float* adv_out, void* stream);
/* The same with a row mask, valid float32 [n] of 0 / 1 (rows are data rows 0 .. n-1): moments = {sum valid adv, sum valid adv^2,
 * sum valid}.  Same 4096-row chunks, fixed summation order and workspace protocol as ppo_adv_moments_ws (one workspace serves both);
 * every chunk's valid rows are moved to its front before they are summed, so all-ones gives the bits of ppo_adv_moments_ws and a
 * minibatch of one chunk gives the bits of ppo_adv_moments_ws on its valid rows alone.  ppo_adv_normalize_masked: invalid rows get 0;
 * a count of 0 gives all zeros, without a division. */
int ppo_adv_moments_masked_ws(const float* returns, const float* values, const float* valid, int n, double* moments, void* workspace,
                              void* stream);
int ppo_adv_normalize_masked(const float* returns, const float* values, const float* valid, int n, const double* moments, float* adv_out,
                             void* stream);

/* Scores of the 'ours' opponent selector (alg_ppo.py:227-244) for ncand (1..32) candidates in ONE launch.  obs [n][obs_stride] and
 * actions [n][ac_dim] are the opponent's samples of the last rollout; ref_params is the net that produced them, table holds frozen
 * nets as rows of table_stride floats in the layout of `params` (matches.SnapshotTable), cand_rows DEVICE int32 [ncand] the rows to
 * score (any order, repeats allowed).  With ap / nap the reference's / a candidate's neglogp of the given action -- the same trunk
 * and the same neglogp expression as ppo_forward, equal to its values bit for bit as tests/test_gpu_selector.py verifies, not by
 * shared code alone -- r = nap / ap - 1 in float32 per row; rows where r is not finite, or whose observation holds a NaN,
 * are left out; score_sum double [ncand] receives the sum of |r| over the others and finite_count int32 [ncand] their number (the
 * selector's score is their quotient).  neglogp_dbg (may be NULL) float32 [ncand + 1][n]: every neglogp, row 0 = the reference net.
 * Deterministic: a fixed summation order for a given n and grid; max_blocks > 0 caps the grid (0 = sized from the device).
 * workspace: ppo_selection_scores_workspace_bytes() bytes, ZERO-INITIALISED once by the caller, one call in flight per workspace.
 * Argument errors (ncand outside 1..32, n < 1, ob_dim / ac_dim outside ppo_forward's range) return before anything is launched. */
size_t ppo_selection_scores_workspace_bytes(void);
int ppo_selection_scores(const float* ref_params, const float* table, int table_stride, const int32_t* cand_rows, int ncand,
                         const float* obs, int n, int obs_stride, int ob_dim, int ac_dim, const float* actions,
                         double* score_sum, int32_t* finite_count, float* neglogp_dbg, int max_blocks, void* workspace, void* stream);

/* Gradient of the PPO loss over minibatch rows idx[0..n): grads float32 [P] receives d(sum-loss)/d(theta) with
 * sum-loss = sum_i w_i*pg_i + vf_coef * sum_i 0.5 (v_i-R_i)^2 - n_local*ent_coef*entropy, where every per-row term
 * is pre-divided by inv_count = 1/global_count (so summing grads over ranks gives the gradient of the global mean loss).
 * stats double[PPO_NSTATS] accumulate the un-normalised sums.  log_ratio_out [n] (minibatch order) may be NULL.
 * workspace: ppo_grad_workspace_bytes(ob_dim, ac_dim) bytes of scratch, ZERO-INITIALISED once by the caller (its tail holds the arrival
 * counters of the in-launch slab reduction, which every call leaves at zero); one ppo_grad in flight per workspace.
 * Environment PPO_GRAD_BLOCKS (1..1024, default 256; read on every call): workgroups per net, i.e. how many 16-row tiles a workgroup walks. */
size_t ppo_grad_workspace_bytes(int ob_dim, int ac_dim);
int ppo_grad(const float* params, const float* obs, int obs_stride, int ob_dim, int ac_dim, const float* actions,
             const float* adv_mb, const float* returns, const float* old_neglogp, const float* is_weight,
             const int32_t* idx, int n, double inv_count, float cliprange, float ent_coef, float vf_coef, float* grads,
             double* stats, float* log_ratio_out, void* workspace, void* stream);

/* ppo_grad for the net the zoo forward evaluates (ppo_forward_filtered with PPO_FWD_TANH on rows that are already filtered): the same
 * objective, row gather, PPO_GRAD_BLOCKS grid, slab reduction, statistics slots, log-ratio output and NaN rules, on the same workspace
 * (ppo_grad_workspace_bytes serves both entries; one gradient launch in flight per workspace).
 *   flags    PPO_GRAD_TANH: tanh hidden units in both trunks (the tanhf of the forward kernel; the backward factor is 1 - h*h of the
 *            stored activation).  0: relu, as ppo_grad.
 *   value    v = v_scale * head + v_shift, the zoo's return-filter de-normalisation (robosumo/robosumo/policy_zoo/policy.py:58-60); the
 *            value loss stays 0.5 (v - R)^2, so the head's delta carries v_scale.
 * With flags = 0, v_scale = 1, v_shift = 0 the call runs ppo_grad's own kernel: gradients, statistics and log-ratios bit for bit.
 * `obs` holds FILTERED rows (ppo_obs_filter, once per update).  Refused before any launch: an unknown flag bit, v_scale not finite or
 * <= 0, v_shift not finite, and whatever ppo_grad refuses. */
#define PPO_GRAD_TANH 1
int ppo_grad_act(const float* params, const float* obs, int obs_stride, int ob_dim, int ac_dim, const float* actions,
                 const float* adv_mb, const float* returns, const float* old_neglogp, const float* is_weight,
                 const int32_t* idx, int n, double inv_count, float cliprange, float ent_coef, float vf_coef, int flags, float v_scale,
                 float v_shift, float* grads, double* stats, float* log_ratio_out, void* workspace, void* stream);

/* out[r][c] = clip((obs[r][c] - mean[c]) * invstd[c], -clip, clip) for r < n, c < ob_dim: the observation filter of the zoo nets with
 * the forward kernel's own expression, for a learner that filters its batch copy once per update.  Columns behind ob_dim are neither
 * read nor written.  out may equal obs when the strides agree.  Refused: n < 1, NULL pointers, clip <= 0, a stride below ob_dim,
 * out == obs with different strides. */
int ppo_obs_filter(const float* obs, int n, int obs_stride, int ob_dim, const float* mean, const float* invstd, float clip,
                   float* out, int out_stride, void* stream);

/* The statistics PPOModel.train returns (model.py:138,205-213) from the sums ppo_grad accumulated: out5 = {policy loss, value loss,
 * entropy, approxkl, clipfrac}; entropy = sum(logstd + 0.5 log(2 pi e)) of the policy the loss was evaluated with
 * (baselines distributions.py:246-247).  logstd float32 [ac_dim] (inside the flat parameter vector), stats double[PPO_NSTATS]. */
int ppo_loss_stats(const double* stats, const float* logstd, int ac_dim, double* out5, void* stream);

/* --- A2C (the reference's ActorCriticModel, model.py:216-372) -------------------------------------------------------------------
 * ppo_a2c_grad: gradient of the A2C loss over rows idx[0..n) (idx may be NULL = identity), on the same MFMA kernel as ppo_grad with
 * the per-row loss swapped at compile time:
 *   sum-loss = sum_i w_i adv_i neglogp_i + vf_coef * sum_i 0.5 w_i (v_i - R_i)^2 - n_local * ent_coef * entropy
 * with every per-row term pre-divided by inv_count = 1 / global_count, as ppo_grad.  No ratio, no clipping; unlike ppo_grad the
 * IS weight multiplies the value term too (model.py:275).  adv [n] is in minibatch order (ppo_adv_normalize's output); obs,
 * actions, returns, is_weight are data rows.  stats double[PPO_NSTATS] accumulate: 0 sum w adv neglogp, 1 sum 0.5 w (v-R)^2,
 * 5 sum w, 6 count; slots 3 and 4 receive 0.  workspace: ppo_grad_workspace_bytes(ob_dim, ac_dim) bytes, ZERO-INITIALISED once by
 * the caller, same contract as ppo_grad (one gradient launch in flight per workspace; ppo_grad and ppo_a2c_grad may share one).
 * ppo_a2c_loss_stats: out3 = {policy_loss, value_loss, policy_entropy} (model.py:296-297) from those sums and logstd [ac_dim]. */
int ppo_a2c_grad(const float* params, const float* obs, int obs_stride, int ob_dim, int ac_dim, const float* actions,
                 const float* adv, const float* returns, const float* is_weight, const int32_t* idx, int n, double inv_count,
                 float ent_coef, float vf_coef, float* grads, double* stats, void* workspace, void* stream);
int ppo_a2c_loss_stats(const double* stats, const float* logstd, int ac_dim, double* out3, void* stream);

/* params -= Adam(clip_by_global_norm(grads, max_grad_norm)); m, v float32 [P]; step t >= 1 (TF1 bias correction).
 * max_grad_norm <= 0 disables clipping.  stats[7] receives the global gradient norm. */
int ppo_clip_adam(float* params, const float* grads, float* m, float* v, int P, int t, double lr, double beta1,
                  double beta2, double eps, double max_grad_norm, double* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
