/* sumo_hip.h -- C ABI of the MI355X-native batched RoboSumo environment engine (libsumo_hip.so).
 *
 * This is the drop-in boundary for the vectorised env step.  The reference has no FFI for this path -- its
 * seam is the Python VecEnv interface -- so each entry point names the reference interface it stands in for:
 *
 *   sumo_create   load_model_from_path + MjSim construction for every worker process
 *                 (reference robosumo/robosumo/envs/mujoco_env.py:55-57, subproc_vec_env.py:49-56)
 *   sumo_reset    SubprocVecEnv.reset -> env.reset() in each worker
 *                 (reference subproc_vec_env.py:78-82, mujoco_env.py:104-108, sumo.py:232-253)
 *   sumo_step     SubprocVecEnv.step_async/step_wait -> worker 'step' incl. auto-reset
 *                 (reference subproc_vec_env.py:10-16,65-76; sumo_env.py:40-72; sumo.py:120-192;
 *                  mujoco_env.py:125-129 -> mj_step x frame_skip, mujoco-py/mujoco_py/mjsim.pyx:115-129)
 *   sumo_get_state / sumo_set_state   MjSim.get_state / set_state (mujoco-py/mujoco_py/mjsim.pyx:247-276)
 *
 * All array arguments of sumo_reset / sumo_step are DEVICE pointers owned by the caller (obs, rewards and
 * dones never leave HBM); sumo_get_state / sumo_set_state take HOST pointers and synchronise.  `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  Every function returns 0 on success and a negative
 * code on error; sumo_last_error() then describes it.  A handle is bound to one GPU; calls on one handle are
 * not re-entrant.
 *
 * Shapes (E = num_envs, A = 2 agents, row-major):
 *   actions  float32 [E][A][act_stride]     raw policy outputs (clamped to ctrlrange inside, as MuJoCo does)
 *   obs      float32 [E][A][obs_stride]     agents.py:190-214 layout + time feature (sumo_env.py:68-70)
 *   info     float64 [E][A][8]              ctrl, lose, win, main, move, push, shaping, flags(bit0 winner, bit1 timeout,
 *                                           bit2 diverged: the state failed MuJoCo's bad-value test -- NaN or |x| > 1e10 in
 *                                           qpos/qvel/qacc, mujoco-py/mujoco_py/builder.py:351-369 raises there -- the step
 *                                           then reports zero rewards, done, and the env auto-resets)
 *   done     uint8   [E][A]
 *   ep_r, ep_dr float64 [E]; ep_l int32 [E] episode return / dense return / length of agent 0, valid where done
 */
#ifndef SUMO_HIP_H
#define SUMO_HIP_H
#include <stddef.h>
#include <stdint.h>
#include "sumo_ppo.h"   /* ppo_lstm_net (sumo_rollout_steps_lstm) */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sumo_engine* sumo_handle_t;

#define SUMO_INFO_STRIDE 8
#define SUMO_NDIMS 16 /* nq nv nu nbody njnt ngeom npair nagent obs_stride act_stride maxcon maxefc lds_bytes state_stride jbcap 0 */

const char* sumo_last_error(void);
int sumo_create(const void* model_blob, size_t nbytes, int num_envs, int device, sumo_handle_t* out);
int sumo_destroy(sumo_handle_t h);
int sumo_dims(sumo_handle_t h, int32_t* out /* [SUMO_NDIMS] */);
int sumo_reset(sumo_handle_t h, const uint64_t* seeds_host /* [E] or NULL */, const uint8_t* mask_dev /* [E] or NULL */,
               float* obs_dev, void* stream);
int sumo_step(sumo_handle_t h, const float* actions_dev, float* obs_dev, double* info_dev, uint8_t* done_dev,
              double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
/* K consecutive self-play rollout steps of every env of the engine in ONE launch: replaces the body of Runner.run's step loop
 * (runner.py:62-151: the five policy / value evaluations, env.step, the reward curriculum, the buffer appends) together with
 * the SubprocVecEnv round trip (subproc_vec_env.py:65-76) for MLP(64,64) policies (policies.py:14-128, baselines models.py:74-103,
 * distributions.py:227-251).  The wavefront that owns an env evaluates the learner's policy and value nets and the opponent's
 * policy net on the env's two observations on the matrix cores, samples both actions (action = mean + exp(logstd) * noise),
 * scores each with the other net, steps the env and appends to the rollout buffers; nothing is launched and no env waits for
 * another between two steps.  Results equal sumo_step + ppo_selfplay_forward + ppo_post_step called step by step, bit for bit.
 *   parameters: flat float32 vectors in the sumo_ppo.h layout; opponent_params holds npool frozen snapshots [npool][P] and
 *     opponent_index[e] (NULL = all 0) selects the snapshot env e plays against (the reference loads ONE snapshot for all envs
 *     per update, alg_ppo.py:213-214: npool = 1)
 *   noise0 / noise1 float32 [T][E][ac_dim]: standard-normal draws for the learner's (agent 0) / the opponent's (agent 1) actions
 *   rollout buffers, agent-major like Runner's mb_* lists: obs [2][T][Ntot][ob_dim], act [2][T][Ntot][ac_dim], rew / val / nlp
 *     (learner's neglogp) / onlp (opponent's neglogp) float32 [2][T][Ntot], done uint8 [2][T][Ntot] (flags BEFORE each step),
 *     ep_done uint8 / ep_r float64 / ep_l int32 [T][Ntot] (agent 0's episode records, monitor.py:63-78); this engine's envs are
 *     columns env_offset .. env_offset + E - 1; steps s0 .. s0 + K - 1 are written
 *   alpha: weight of the shaping reward (runner.py:130-134)
 * The env-side buffers are those of sumo_step (actions is written: it receives the sampled actions).  Launches of one engine must
 * be ordered on one stream (the engine owns the launch's ticket / progress counters); different engines may run concurrently.
 * After the launch obs / done hold the state after the last step as after sumo_step; info / ep_* hold the last step's values. */
typedef struct sumo_rollout {
  const float* learner_params;
  const float* opponent_params;
  const int32_t* opponent_index;
  int npool, ob_dim, ac_dim;
  int T, Ntot, env_offset, s0, K;
  double alpha;
  const float *noise0, *noise1;
  float *obs, *act, *rew, *val, *nlp, *onlp;
  uint8_t *done, *ep_done;
  double* ep_r;
  int32_t* ep_l;
} sumo_rollout;
int sumo_rollout_steps(sumo_handle_t h, const sumo_rollout* r, float* actions_dev, float* obs_dev, double* info_dev, uint8_t* done_dev,
                       double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);

/* The same launch for RECURRENT policies (learn(network='lstm'): baselines lstm(128), value head on the same latent;
 * Runner's recurrent branch = reference runner.py:62-96 with the S / M feeds of models.py:163-170).  Per step and env the wave
 * evaluates: learner(obs 0, state0) -> action 0 / neglogp / value / new state0; opponent(obs 0, zero state) -> its likelihood of
 * action 0; opponent(obs 1, state1) -> action 1 / its neglogp / new state1; learner(obs 1, NEW state1) -> the value recorded for
 * agent 1; learner(obs 1, zero state) -> its likelihood of action 1.  State rows are zeroed where the previous step's done flag
 * is set before a cell runs.  Numbers equal the ppo_lstm_step launches of the step-by-step path bit for bit.
 *   learner        HOST struct (device pointers inside): hidden 128, gate order i,f,o,u, no embedding / observation filter
 *   opponents_dev  DEVICE array of npool structs of the same shape; tile_net_dev DEVICE int32 [Ntot / 16]: the snapshot every
 *                  16-env tile of the WHOLE env set faces (tile of env e of this engine: (env_offset + e) / 16), NULL = snapshot 0
 *   state0/state1  DEVICE float32 [E][256] (c | h): recurrent state of agent 0's / agent 1's acting net, rows of THIS engine's
 *                  envs; read at step s0, left at the state after step s0 + K - 1
 * Everything else as sumo_rollout.  Ordering contract as sumo_rollout_steps. */
typedef struct sumo_rollout_lstm {
  const ppo_lstm_net* learner;
  const ppo_lstm_net* opponents_dev;
  const int32_t* tile_net_dev;
  int npool;
  float *state0, *state1;
  int T, Ntot, env_offset, s0, K;
  double alpha;
  const float *noise0, *noise1;
  float *obs, *act, *rew, *val, *nlp, *onlp;
  uint8_t *done, *ep_done;
  double* ep_r;
  int32_t* ep_l;
} sumo_rollout_lstm;
int sumo_rollout_steps_lstm(sumo_handle_t h, const sumo_rollout_lstm* r, float* actions_dev, float* obs_dev, double* info_dev,
                            uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
/* sumo_rollout_steps_lstm for OPPONENT-DATA REUSE by a recurrent learner (learn(network='lstm', use_opponent_data=...)): agent 1's
 * samples join the update batch, and BPTT re-evaluates them along agent 1's sequence with the LEARNER's net.  So the learner carries a
 * state of its own along agent 1's stream, the shadow state, and the launch records agent 1's value and the learner's neglogp of
 * action 1 from it: learner(obs 1, state2 masked by agent 1's done flag of the previous step) -> val[1], nlp[1], new state2.  That one
 * evaluation replaces the last two of sumo_rollout_steps_lstm (value from agent 1's NEW opponent state, neglogp from a zero state);
 * every other number of the launch -- actions, agent 0's record, onlp, state0, state1, the env -- is that launch's, bit for bit.
 *   ro       the launch struct of sumo_rollout_steps_lstm, every field as there
 *   state2   DEVICE float32 [E][256] (c | h): the shadow state, rows of THIS engine's envs; read at step s0, left at the state after
 *            step s0 + K - 1
 * Numbers equal the step-by-step path (Runner._step_group with reuse_opponent) bit for bit.  Refused: whatever sumo_rollout_steps_lstm
 * refuses (hidden other than 128, a window outside the rollout buffers, ...), a missing state2.  Ordering contract as there. */
typedef struct sumo_rollout_lstm_reuse {
  sumo_rollout_lstm ro;
  float* state2;
} sumo_rollout_lstm_reuse;
int sumo_rollout_steps_lstm_reuse(sumo_handle_t h, const sumo_rollout_lstm_reuse* r, float* actions_dev, float* obs_dev, double* info_dev,
                                  uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
/* K consecutive steps of checkpoint-vs-checkpoint MATCHES of every env of the engine in ONE launch: replaces the step loop of the
 * reference's compare_history_version.py:16-47 / play_evaluation.py (model[0].step on obs 0, model[1].step on obs 1, env.step, the
 * winner bookkeeping) for MLP(64,64) policies, on the fused launch of sumo_rollout_steps (same scheduler, hand-over and env step).
 * The wavefront that owns env e evaluates two policy trunks: snapshot idx0[e] acts for agent 0 on obs 0, snapshot idx1[e] for
 * agent 1 on obs 1 (idx0[e] == idx1[e] is allowed); no value net, no cross-scoring, no rollout buffer.
 *   params    float32 [nsnap][P] flat parameter vectors in the sumo_ppo.h layout; idx0 / idx1 int32 [E] (DEVICE) select each env's
 *             snapshots -- an index outside [0, nsnap) raises the launch's abort flag (sumo_rollout_status returns -20)
 *   noise0 / noise1  float32 [T][E][ac_dim] standard-normal draws: action = mean + exp(logstd) * noise (PPOModel.step); both NULL =
 *             deterministic play, action = mean (PPOModel.step(deterministic=True)); steps s0 .. s0 + K - 1 are read
 *   score     int32 [E][3] = {agent-0 wins, agent-1 wins, draws}, read and updated in place: where agent 0's episode ends in a step, a
 *             win if agent 0 carries the winner flag (info[.][0][7] bit 0), a loss if only agent 1 does, a draw otherwise; counted
 *             while wins + losses + draws < quota (compare_history_version.py:33-41, eval_robosumo_against_fix.py's rule)
 * The env-side buffers are those of sumo_step (actions receives both actions), left as after the last step.  Ordering contract as
 * sumo_rollout_steps; the outcome is read with sumo_rollout_status.  Refused: cfrc_mode rne_post, mixed match-ups (ob_dim / ac_dim
 * differing between the sides), nsnap < 1, ob_dim / ac_dim other than the scene's. */
typedef struct sumo_match {
  const float* params;
  const int32_t *idx0, *idx1;
  int nsnap, ob_dim, ac_dim;
  int T, s0, K, quota;
  const float *noise0, *noise1;
  int32_t* score;
} sumo_match;
int sumo_match_steps(sumo_handle_t h, const sumo_match* m, float* actions_dev, float* obs_dev, double* info_dev, uint8_t* done_dev,
                     double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
/* The same matches for RECURRENT checkpoints (LstmPPOModel.save, learn(network='lstm')): agent g in {0, 1} acts with net
 * nets_dev[idx_g[e]] on (obs g, its own state state_g[e]), the state row zeroed first where agent g's done flag of the previous step
 * is set -- LstmPPOModel.step(obs, S, M) on one row, bit for bit.  No value head is read.
 *   proto      HOST struct: the dimensions / gate order every net of the table shares; checked as sumo_rollout_lstm's learner (hidden
 *              128, gate order i,f,o,u, no embedding / observation filter, wx / wh / b / head_w / head_b / logstd present)
 *   nets_dev   DEVICE array of nsnap ppo_lstm_net structs of that shape; idx0 / idx1 int32 [E] (DEVICE) select each env's nets -- an
 *              index outside [0, nsnap) raises the launch's abort flag (sumo_rollout_status returns -20)
 *   state0/state1  DEVICE float32 [E][256] (c | h) per agent, read at step s0 and left at the state after step s0 + K - 1 (the
 *              caller zeroes them where a match-up starts)
 *   noise0 / noise1, score, quota, T / s0 / K  as sumo_match (action = mean + exp(logstd) * noise, or the mean when both are NULL)
 * Refused: whatever sumo_match_steps refuses, a proto sumo_rollout_steps_lstm would refuse, missing state buffers. */
typedef struct sumo_match_lstm {
  const ppo_lstm_net* proto;
  const ppo_lstm_net* nets_dev;
  const int32_t *idx0, *idx1;
  int nsnap;
  float *state0, *state1;
  int T, s0, K, quota;
  const float *noise0, *noise1;
  int32_t* score;
} sumo_match_lstm;
int sumo_match_steps_lstm(sumo_handle_t h, const sumo_match_lstm* m, float* actions_dev, float* obs_dev, double* info_dev,
                          uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
/* The fused launches against POLICY-ZOO MLP nets (the reference's robosumo/policy_zoo MLPPolicy(normalize=True), policy.py:23-91:
 * tanh 64-64 trunks, running-mean observation filter clipped to +-obs_clip, input = the first ob_dim observation columns -- the
 * observation without the time feature, eval_robosumo_against_fix.py:206).  A table of nzoo frozen nets of one ob_dim:
 *   params  float32 [nzoo][Pz] flat vectors in the sumo_ppo.h layout for (ob_dim, the scene's ac_dim), Pz = ppo_param_count(ob_dim,
 *           ac_dim): pi trunk, vf trunk (never read here), pi head, logstd, vf head
 *   filt    float32 [nzoo][2][ob_dim]: the observation filter's mean | 1 / std (std = sqrt(max(var, 1e-2)), utils.py:30-32)
 * The owning wave evaluates a zoo net as ppo_forward_filtered does (clip((x - mean) / std, +-obs_clip), tanh trunk, Gaussian head),
 * bit for bit.  Zoo LSTM nets (policy.py:94-199) are not played by these two entry points: see sumo_zoo_lstm below.
 *
 * sumo_rollout_steps_zoo: sumo_rollout_steps with agent 1 played by a zoo net (learn(opponent_mode='fix'), reference
 *   alg_ppo.py:194-206): per step and env the learner's policy and value nets on both observations, zoo net opponent_index[e]
 *   (NULL = net 0) on both; the learner samples action 0 and the zoo net scores it, the zoo net samples action 1 (mean + exp(logstd)
 *   * noise1) and the learner scores and values it; the zoo net's value trunk is not evaluated.  r->opponent_params must be NULL and
 *   r->npool == z->nzoo; an opponent_index outside [0, nzoo) raises the launch's abort flag (sumo_rollout_status returns -20).
 *   Everything else as sumo_rollout_steps.
 * sumo_match_steps_zoo: sumo_match_steps with agent 1 played by zoo nets (eval_robosumo_against_fix.py:196-230): agent 0 acts with
 *   checkpoint m->idx0[e] of m->params [m->nsnap][P], agent 1 with zoo net m->idx1[e] of z; noise, score, quota and the abort on a
 *   bad index (idx0 against nsnap, idx1 against nzoo) as sumo_match_steps.
 * Refused: whatever the sibling entry point refuses, ob_dim outside [1, the scene's ob_dim], nzoo < 1, missing params / filt,
 * obs_clip <= 0. */
typedef struct sumo_zoo_mlp {
  const float* params;
  const float* filt;
  float obs_clip;   /* 5 for the zoo nets */
  int nzoo, ob_dim;
} sumo_zoo_mlp;
int sumo_rollout_steps_zoo(sumo_handle_t h, const sumo_rollout* r, const sumo_zoo_mlp* z, float* actions_dev, float* obs_dev,
                           double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
int sumo_match_steps_zoo(sumo_handle_t h, const sumo_match* m, const sumo_zoo_mlp* z, float* actions_dev, float* obs_dev,
                         double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
/* The fused match launches against POLICY-ZOO LSTM nets (the reference's robosumo/policy_zoo LSTMPolicy(normalize=True),
 * policy.py:94-199: observation filter clipped to +-obs_clip on the first ob_dim observation columns, relu embedding of emb_dim,
 * BasicLSTMCell(hidden) in gate order i,j,f,o with forget_bias, Gaussian head; two such branches, of which only the POLICY branch
 * -- p/emb, lstmp, p/out, logstd -- is evaluated, as ZooLSTMPolicy.act does without want_value).  A table of nzoo frozen nets of one
 * ob_dim, emb_dim = hidden = 64:
 *   params  float32 [nzoo][Pz], each row in this order (A = the scene's ac_dim):
 *             emb_w  [ob_dim][64]      p/emb/w
 *             emb_b  [64]              p/emb/b
 *             kernel [64 + 64][256]    lstmp/kernel: the 64 input rows, then the 64 recurrent rows; columns gate-major i | j | f | o
 *             bias   [256]             lstmp/bias (forget_bias is added to the f block inside)
 *             head_w [64][A]           p/out/w
 *             head_b [A]               p/out/b
 *             logstd [A]
 *           Pz = 64 ob_dim + 64 + 128 * 256 + 256 + 64 A + 2 A
 *   filt    float32 [nzoo][2][ob_dim]: the observation filter's mean | 1 / std, as sumo_zoo_mlp
 *   state   float32 [E][2 * 64] (c | h): agent 1's recurrent state, rows of THIS engine's envs; read at step s0, left at the state
 *           after step s0 + K - 1 (the caller zeroes it where a match-up starts).  Inside the launch a row is zeroed before the cell
 *           runs where AGENT 0's done flag of the previous step is set (policy_zoo._evaluate_against resets the opponent on it).
 * The owning wave evaluates the net as ppo_lstm_step does with a ppo_lstm_net filled like ZooLSTMPolicy's policy branch, bit for bit.
 *
 * sumo_match_steps_zoo_lstm: sumo_match_steps_zoo with agent 1 played by zoo LSTM nets: agent 0 acts with MLP(64,64) checkpoint
 *   m->idx0[e] of m->params [m->nsnap][P], agent 1 with net m->idx1[e] of z.
 * sumo_match_steps_lstm_zoo_lstm: the same for RECURRENT checkpoints: agent 0 is agent 0 of sumo_match_steps_lstm (net m->idx0[e] of
 *   m->nets_dev on its state m->state0, LSTM(128)); m->state1 must be NULL (agent 1's state is z->state).
 * Two entry points rather than a mode field, like the MLP / LSTM pair of sumo_match_steps: each takes its sibling's launch struct.
 * Noise (m->noise0 for agent 0, m->noise1 for agent 1; both NULL = deterministic), score, quota and the abort on a bad index (idx0
 * against nsnap, idx1 against nzoo: sumo_rollout_status returns -20, row 0 plays) as sumo_match_steps.  Refused: whatever the sibling
 * entry point refuses, ob_dim outside [1, the scene's ob_dim], nzoo < 1, missing params / filt / state, obs_clip <= 0, emb_dim /
 * hidden other than 64, a scene whose policy scratch cannot hold the observation tile plus the embedding and latent rows. */
typedef struct sumo_zoo_lstm {
  const float* params;
  const float* filt;
  float* state;
  float obs_clip;      /* 5 for the zoo nets */
  float forget_bias;   /* 1 for the zoo nets (tf BasicLSTMCell) */
  int nzoo, ob_dim, emb_dim, hidden;
} sumo_zoo_lstm;
int sumo_match_steps_zoo_lstm(sumo_handle_t h, const sumo_match* m, const sumo_zoo_lstm* z, float* actions_dev, float* obs_dev,
                              double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
int sumo_match_steps_lstm_zoo_lstm(sumo_handle_t h, const sumo_match_lstm* m, const sumo_zoo_lstm* z, float* actions_dev, float* obs_dev,
                                   double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev,
                                   void* stream);
/* CROSS-FAMILY checkpoint matches: an MLP(64,64) run against an LSTM(128) run (which of `run.py --network mlp` and `--network lstm`
 * wins?).  Agent lstm_side acts as that agent of sumo_match_steps_lstm does -- net nets_dev[idx_g[e]] on (obs g, state[e]), the state
 * row zeroed first where ITS done flag of the previous step is set, LstmPPOModel.step(obs, S, M) -- and the other agent as that agent
 * of sumo_match_steps does (checkpoint idx_g[e] of params, PPOModel.step); every number of a side equals ppo_lstm_step / ppo_forward
 * bit for bit.
 *   params, nsnap_mlp, ob_dim, ac_dim   the MLP side's table [nsnap_mlp][P], as sumo_match
 *   proto, nets_dev, nsnap_lstm         the LSTM side's table, as sumo_match_lstm
 *   state      DEVICE float32 [E][256] (c | h) of the recurrent agent, read at step s0 and left at the state after step s0 + K - 1
 *   lstm_side  0 or 1: the agent the LSTM table plays, for every env of the launch; idx0 / idx1 [E] index the table of THEIR agent,
 *              and each is checked against its own table's size (an index outside it raises the abort flag: sumo_rollout_status
 *              returns -20, row 0 plays)
 *   noise0 / noise1, score, quota, T / s0 / K  as sumo_match
 * Refused: whatever sumo_match_steps and sumo_match_steps_lstm refuse for their halves (cfrc_mode rne_post, mixed match-ups, ob_dim
 * / ac_dim other than the scene's, a proto of another shape, missing buffers, one noise pointer without the other), lstm_side
 * outside {0, 1}, a missing state, nsnap_mlp or nsnap_lstm below 1, a scene whose per-step LDS area cannot hold the observation tile
 * plus the larger of the latent rows and the MLP trunk's hidden tiles. */
typedef struct sumo_match_cross {
  const float* params;
  int nsnap_mlp, ob_dim, ac_dim;
  const ppo_lstm_net* proto;
  const ppo_lstm_net* nets_dev;
  int nsnap_lstm;
  float* state;
  int lstm_side;
  const int32_t *idx0, *idx1;
  int T, s0, K, quota;
  const float *noise0, *noise1;
  int32_t* score;
} sumo_match_cross;
int sumo_match_steps_cross(sumo_handle_t h, const sumo_match_cross* m, float* actions_dev, float* obs_dev, double* info_dev,
                           uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
/* sumo_match_steps_lstm_zoo: LSTM(128) checkpoints (agent 0) against policy-zoo MLP nets (agent 1) -- eval_robosumo_against_fix.py's
 *   games for a recurrent run against the reference's default opponent.  Agent 0 is agent 0 of sumo_match_steps_lstm (net m->idx0[e]
 *   of m->nets_dev on its state m->state0) and reads the raw observation first; agent 1 is agent 1 of sumo_match_steps_zoo (zoo net
 *   m->idx1[e] of z on the tile filtered in place, ppo_forward_filtered bit for bit).  m->state1 must be NULL (a zoo MLP net has no
 *   state).  Noise, score, quota and the abort on a bad index (idx0 against nsnap, idx1 against nzoo) as sumo_match_steps.  Refused:
 *   whatever sumo_match_steps_lstm refuses, state1 given, and the table z exactly as sumo_match_steps_zoo refuses it. */
int sumo_match_steps_lstm_zoo(sumo_handle_t h, const sumo_match_lstm* m, const sumo_zoo_mlp* z, float* actions_dev, float* obs_dev,
                              double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
/* sumo_rollout_steps_zoo_lstm: sumo_rollout_steps_zoo with agent 1 played by a zoo LSTM net (learn(opponent_mode='fix') with an
 *   LSTM file): per step and env the learner's MLP(64,64) policy and value nets on both observations; the learner samples action 0;
 *   zoo net r->opponent_index[e] of z (NULL = net 0) acts on agent 1's observation from the env's row of z->state, which is zeroed
 *   first where AGENT 1's done flag of the previous step is set (the Runner's M = dones[:, 1]) and left at the new state; its action
 *   is mean + exp(logstd) * noise1 and its neglogp goes to onlp[1].  The same net then scores action 0 on agent 0's observation
 *   from a ZERO state (one cell evaluation, no state written) for onlp[0], as the Runner's scoring calls feed no state; the learner
 *   scores and values action 1.  The record holds the raw observations.  z->state: [E][2 * 64] rows of this engine's envs.
 *   Every recorded number equals ppo_forward (learner) / ppo_lstm_step (zoo net) bit for bit.
 *   Refused: r->opponent_params != NULL, r->npool != z->nzoo, and whatever sumo_rollout_steps (cfrc_mode rne_post, mixed match-ups,
 *   ...) and the zoo LSTM match launches (ob_dim outside [1, the scene's ob_dim], nzoo < 1, missing params / filt / state,
 *   obs_clip <= 0, emb_dim / hidden other than 64) refuse.  An opponent_index outside [0, nzoo) raises the launch's abort flag
 *   (sumo_rollout_status returns -20) and plays row 0. */
int sumo_rollout_steps_zoo_lstm(sumo_handle_t h, const sumo_rollout* r, const sumo_zoo_lstm* z, float* actions_dev, float* obs_dev,
                                double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
/* The rollout launches of a RECURRENT learner against policy-zoo nets (learn(network='lstm', opponent_mode='fix')): the launch
 * struct of sumo_rollout_steps_lstm with agent 1 played by a zoo net of the table z.  Per step and env the owning wave evaluates
 *   learner(obs 0, state0)    -> action 0 (mean + exp(logstd) * noise0) / neglogp / value / new state0; the state row is zeroed
 *                                first where AGENT 0's done flag of the previous step is set
 *   zoo net on obs 0          -> its likelihood of action 0 (onlp[0]); an LSTM net: one cell evaluation from a ZERO state, no state
 *                                written
 *   zoo net on obs 1          -> action 1 (mean + exp(logstd) * noise1) and its neglogp (onlp[1]); an LSTM net acts from the env's
 *                                row of z->state, zeroed first where AGENT 1's done flag of the previous step is set, and leaves
 *                                the new state there
 *   learner(obs 1, ZERO state) -> its likelihood (nlp[1]) AND the value (val[1]) of action 1, ONE cell evaluation: a zoo net's
 *                                state is not the learner's, so the rule of sumo_rollout_steps_lstm (value from agent 1's new
 *                                state) has nothing to feed
 * The record holds the raw observations.  Every recorded number equals the ppo_lstm_step (learner, zoo LSTM net) /
 * ppo_forward_filtered (zoo MLP net) launches of the step-by-step path bit for bit.
 *   r->learner, r->state0   as sumo_rollout_steps_lstm (hidden 128, gate order i,f,o,u; [E][256] rows of THIS engine's envs)
 *   r->opponents_dev, r->state1   must be NULL; r->npool == z->nzoo
 *   r->tile_net_dev   DEVICE int32 [Ntot / 16]: the table row every 16-env tile of the WHOLE env set faces, exactly as it selects
 *                     the snapshot in sumo_rollout_steps_lstm (NULL = row 0); a row outside [0, nzoo) raises the launch's abort flag
 *                     (sumo_rollout_status returns -20) and row 0 plays
 *   z                 sumo_rollout_steps_lstm_zoo: a sumo_zoo_mlp table; sumo_rollout_steps_lstm_zoo_lstm: a sumo_zoo_lstm table
 *                     whose state ([E][2 * 64], rows of this engine's envs) is read at step s0 and left at the state after step
 *                     s0 + K - 1
 * Refused before any launch: whatever sumo_rollout_steps_lstm refuses (cfrc_mode rne_post, mixed match-ups, a learner of another
 * shape, missing buffers, a scene whose per-step LDS area cannot hold the policy scratch, ...), opponents_dev / state1 given,
 * npool != nzoo, and whatever sumo_rollout_steps_zoo / sumo_rollout_steps_zoo_lstm refuse of the table (ob_dim outside [1, the
 * scene's ob_dim], nzoo < 1, missing params / filt / state, obs_clip <= 0, emb_dim / hidden other than 64, cell rows that do not
 * fit the policy scratch).  Ordering contract as sumo_rollout_steps. */
int sumo_rollout_steps_lstm_zoo(sumo_handle_t h, const sumo_rollout_lstm* r, const sumo_zoo_mlp* z, float* actions_dev, float* obs_dev,
                                double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
int sumo_rollout_steps_lstm_zoo_lstm(sumo_handle_t h, const sumo_rollout_lstm* r, const sumo_zoo_lstm* z, float* actions_dev, float* obs_dev,
                                     double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev,
                                     void* stream);
/* The rollout launches against a LEAGUE of policy-zoo nets of both families (learn(opponent_mode='fix', fix_opponent_path=[files])
 * with MLP and LSTM files mixed): every 16-env tile of the whole env set faces one member, MLP tiles and LSTM tiles in one launch.
 *   mlp             a sumo_zoo_mlp table (nzoo >= 1)
 *   lstm            a sumo_zoo_lstm table (nzoo >= 1) whose state ([E][2 * 64]) holds rows of THIS engine's envs; only the envs of
 *                   tiles that face an LSTM member read and write their rows
 *   tile_entry_dev  DEVICE int32 [Ntot / 16], indexed (env_offset + e) / 16 like tile_net_dev (NULL = entry 0): an entry in
 *                   [0, mlp.nzoo) is that row of the MLP table, an entry in [mlp.nzoo, mlp.nzoo + lstm.nzoo) is row
 *                   entry - mlp.nzoo of the LSTM table; any other entry raises the launch's abort flag (sumo_rollout_status returns
 *                   -20) and entry 0 plays
 * The owning wave reads its tile's entry once per step and takes a wave-uniform branch: the zoo pass of sumo_rollout_steps_zoo /
 * sumo_rollout_steps_lstm_zoo (MLP member) or of sumo_rollout_steps_zoo_lstm / sumo_rollout_steps_lstm_zoo_lstm (LSTM member), so
 * every recorded number of a tile equals the single-table launch against its member bit for bit.
 * sumo_rollout_steps_zoo_league: an MLP(64,64) learner (the launch struct of sumo_rollout_steps_zoo; opponent_params and
 *   opponent_index must be NULL).  sumo_rollout_steps_lstm_zoo_league: an LSTM(128) learner (the launch struct of
 *   sumo_rollout_steps_lstm_zoo; opponents_dev, tile_net_dev and state1 must be NULL).  r->npool == mlp.nzoo + lstm.nzoo.
 * Refused before any launch: whatever the sibling launches refuse of the launch struct and of either table (a table with no net
 * included: a league of one family plays through that family's launch), npool other than the league's size, tile_entry_dev with an
 * env range off the 16-env grid, a scene whose policy scratch cannot hold the larger of the two zoo passes. */
typedef struct sumo_zoo_league {
  sumo_zoo_mlp mlp;
  sumo_zoo_lstm lstm;
  const int32_t* tile_entry_dev;
} sumo_zoo_league;
int sumo_rollout_steps_zoo_league(sumo_handle_t h, const sumo_rollout* r, const sumo_zoo_league* z, float* actions_dev, float* obs_dev,
                                  double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
int sumo_rollout_steps_lstm_zoo_league(sumo_handle_t h, const sumo_rollout_lstm* r, const sumo_zoo_league* z, float* actions_dev,
                                       float* obs_dev, double* info_dev, uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev,
                                       int32_t* ep_l_dev, void* stream);
/* K consecutive CO-TRAINING rollout steps on a match-up whose two sides may be different species (RoboSumo-Ant-vs-Bug-v0, ...: two
 * observation widths, two action widths) in ONE launch: what co_train.PairRunner runs per step as ppo_mixed_pair_step + sumo_step +
 * ppo_post_step.  Each side is a seat: a device table of MLP(64,64) + copy-value rows, one row per 16-env tile.  The wave that owns an
 * env evaluates both seats on their own observation, samples both actions (action = mean + exp(logstd) * noise), steps the env and
 * writes rewards and agent 0's episode record as sumo_rollout_steps does.
 *   Side s RECORDS on the tiles whose row equals record_row (-1: on every tile): there its value net runs too and obs / act / nlp / val
 *   and done (that agent's OWN flag before the step) are written at [step][env_offset + e]; on every other tile only its policy net runs
 *   and nothing of the side is written -- the co-training runner lets each learner record on the half of the tiles its live row plays.
 *   A tile_row entry outside [0, nrows) raises the launch's abort flag (sumo_rollout_status returns -20) and row 0 plays.
 * Per env and step each side's action, neglogp and value are the bits of ppo_forward(row, obs_s, PPO_FWD_PI | PPO_FWD_VF, noise_s); env,
 * rewards and episode record are sumo_step's and ppo_post_step's.  Ordering contract and env-side buffers as sumo_rollout_steps.
 * Refused, each with its own code, before anything is launched: cfrc_mode rne_post (-12), steps (-5) or envs (-6) outside the buffers,
 * ob_dim / ac_dim that are not that agent's of the scene (-4), ac_dim above 16 (-16), nrows < 1 (-7), row_stride below
 * ppo_param_count (-17), a missing table (-13), noise (-14), record (-15) or shared buffer (-2), tile_row with env_offset or the env
 * count off the 16-env grid (-11), a scene whose mass-matrix region cannot hold the scratch (-8).  A homogeneous scene is valid. */
typedef struct sumo_pair_side {
  const float* table;          /* DEVICE [nrows][row_stride]: MLP(64,64) + copy-value rows, ppo_forward's flat order */
  const int32_t* tile_row;     /* DEVICE [Ntot / 16]: the row of every 16-env tile of the WHOLE env set; NULL = row 0 */
  int nrows, row_stride, ob_dim, ac_dim;
  int record_row;              /* record (and value) on tiles whose row equals it; -1 = on every tile */
  const float* noise;          /* DEVICE [T][Ntot][ac_dim] */
  float *obs, *act, *val, *nlp; /* DEVICE [T][Ntot][ob_dim], [T][Ntot][ac_dim], [T][Ntot], [T][Ntot] */
  uint8_t* done;               /* DEVICE [T][Ntot] */
} sumo_pair_side;
typedef struct sumo_rollout_pair {
  sumo_pair_side side[2];
  int T, Ntot, env_offset, s0, K;
  double alpha;
  float* rew;                  /* DEVICE [2][T][Ntot] */
  uint8_t* ep_done;            /* DEVICE [T][Ntot], as ep_r (float64) and ep_l (int32) */
  double* ep_r;
  int32_t* ep_l;
} sumo_rollout_pair;
int sumo_rollout_steps_pair(sumo_handle_t h, const sumo_rollout_pair* r, float* actions_dev, float* obs_dev, double* info_dev,
                            uint8_t* done_dev, double* ep_r_dev, double* ep_dr_dev, int32_t* ep_l_dev, void* stream);
/* cfrc_mode (reference agents.py:190-214 reads sim.data.cfrc_ext into 84 of the 121 observation entries):
 *   0 = zero (default): what the reference produces -- its MuJoCo 2.1 scenes declare no force / torque / accelerometer sensor, so
 *       mj_rnePostConstraint never runs and cfrc_ext stays at its reset value 0;
 *   1 = rne_post: the entries as a MuJoCo 2.1 with such a sensor would fill them: |clip(cfrc_ext, +-100)| with cfrc_ext = per-body sum
 *       of the contact wrenches ([torque about the subtree CoM of the body's root ; force], world axes; -wrench on the contact's
 *       first body, + on its second) of the forward evaluation that OPENS the last mj_step of the env step (sensors are evaluated
 *       once per mj_step at its start state; the RK4 sub-stages skip them).  sumo_step then issues a second launch that re-derives
 *       that state from the pre-step state (frame_skip - 1 sub-steps), so a step costs ~1.85x; sumo_rollout_steps* refuse the mode
 *       (the policies read the observations inside their launch).  Envs whose episode ended in the step show the zeros of the reset
 *       observation.  Parity: against the oracle's restatement of mj_rnePostConstraint (unpinned: no MuJoCo here).
 * sumo_get_cfrc_ext: HOST float64 [E][nbody][6] of the last step (mode 1). */
int sumo_set_cfrc_mode(sumo_handle_t h, int mode);
/* Agent._adjust_z (reference robosumo/robosumo/envs/agents.py:33,155-161): a constant added to the torso height an agent REPORTS --
 * get_qpos() returns a copy with qpos[2] += _adjust_z, so it shifts the own-z entry (index 2) and the opponent-z entry (index
 * nq + nv + 6 nbody + 2) of every observation (agents.py:190-214) and both lose tests (sumo.py:147-160: z + adjust_z < 0.29); the
 * physics state, the xy used by the rewards and sumo_get_state are untouched.  0 (default) = training (run.py:76-77 leaves it
 * commented out); the reference's evaluation / play scripts set -0.5 on every agent (eval_robosumo_against_fix.py:108-115,
 * play_fixed.py:23, compare_history_version.py:74): the policy-zoo nets were trained with the tatami surface at z = 0, this fork's
 * is at z = 0.5.  Applies to sumo_reset / sumo_step / sumo_rollout_steps* alike from the next launch on (synchronises). */
int sumo_set_adjust_z(sumo_handle_t h, double adjust_z);
int sumo_get_cfrc_ext(sumo_handle_t h, double* out);
int sumo_get_state(sumo_handle_t h, double* qpos, double* qvel, double* warm, int32_t* counters /* [E][2] */);
int sumo_set_state(sumo_handle_t h, const double* qpos, const double* qvel, const double* warm,
                   const int32_t* counters);
/* A complete snapshot of the envs: everything a later sumo_step / sumo_rollout_steps* output depends on, as one versioned HOST blob
 * (DESIGN.md section 32).  Header (SUMO_SNAPSHOT_HEADER_BYTES): magic, version, E, state_stride, nq, nv, cfrc_mode, the fused-launch
 * count (the hand-over tags in the counters derive from it), adjust_z, a 64-bit FNV-1a hash of the model blob, the payload size.
 * Payload: the state rows [E][state_stride] float64 whole (qpos, qvel, warm start, the episode accumulators), all four counter words
 * [E][4] int32, the per-env seeds [E] uint64 and, in cfrc_mode 1, the pre-step state [E][state_stride] and cfrc_ext [E][nbody][6].
 * Not in it: the fault counters of sumo_stats (a restored engine keeps its own) and what only orders the work (the longest-first
 * schedule, the ticket counters).  Both calls take HOST pointers and synchronise like sumo_get_state / sumo_set_state.
 * sumo_snapshot_load checks everything before it writes anything to the device, each mismatch with its own code and message:
 * -1 NULL pointer, -30 fewer bytes than a header, -31 bad magic, -32 unknown version, -33 another E, -34 another state_stride / nq /
 * nv, -35 another model (hash), -36 another cfrc_mode, -37 fewer bytes than header + payload, -38 a header whose adjust_z is not
 * finite (sumo_snapshot_save: -30 where `bytes` is below sumo_snapshot_bytes).  It applies the header's adjust_z as sumo_set_adjust_z
 * does. */
#define SUMO_SNAPSHOT_MAGIC 0x50414E534F4D5553ull /* "SUMOSNAP" */
#define SUMO_SNAPSHOT_VERSION 1
#define SUMO_SNAPSHOT_HEADER_BYTES 64
size_t sumo_snapshot_bytes(sumo_handle_t h);
int sumo_snapshot_save(sumo_handle_t h, void* dst_host, size_t bytes);
int sumo_snapshot_load(sumo_handle_t h, const void* src_host, size_t bytes);
/* debug / parity hook: run mj_forward once per env at its current state with ctrl (HOST float64 [E][nu]) and return
 * qacc (HOST float64 [E][nv]) plus per-env {ncon, nefc, newton iterations, dropped contacts} (HOST int32 [E][4]). */
int sumo_debug_forward(sumo_handle_t h, const double* ctrl, double* qacc, int32_t* counts);
/* Outcome of the engine's most recent sumo_rollout_steps* launch; waits for that launch (its stream) to finish.
 * A MuJoCo fault is loud in the reference (mujoco-py/mujoco_py/builder.py:351-369 raises MujocoException out of env.step); so is a
 * fused launch that did not complete: returns -20 (sumo_last_error() says why) when the launch's abort flag is set -- a wave's bounded
 * wait for its env's previous step expired, or the record a wave took over did not carry the sequence tag / checksum its writer
 * published (every hand-over is checked) -- and 0 otherwise.  After -20 the rollout buffers hold unwritten rows and the env states
 * are partly advanced: reset before continuing.  out4 (HOST, may be NULL): {abort flag, tickets drawn, tickets of the launch
 * (E x K), hand-over mismatches since creation}.  Runner.run (device mode) and bench.py call this after every rollout. */
int sumo_rollout_status(sumo_handle_t h, int64_t* out4);
/* 1 if this engine runs the static-Layout kernel variants: for the flagship scene (RoboSumo-Ant-vs-Ant-v0, default settings) the LDS
 * layout, the model's dimensions / table offsets and the derived-table offsets are compile-time constants of the per-step and the fused
 * rollout kernels (csrc/layout_static.h, generated by tools/gen_static_layout.py from the engine's own host code; sumo_create compares
 * the scene's runtime values with the tables word for word).  Results agree with the runtime-Layout variants every other scene uses
 * (SUMO_STATIC_LAYOUT=0 forces those) to float64 rounding -- a different compilation of the same source: literals change which multiply-add
 * pairs are contracted -- and the oracle parity tests run on the static variants; 0 otherwise. */
int sumo_static_layout(sumo_handle_t h);
/* The three exports below are host only (no device, no HIP call): each runs the scene preparation of sumo_create itself (parse, derived
 * tables and lane records, Layout, lane role words, final checks; settings from the SUMO_* environment variables read once) and stops
 * after the stage it reports, so what they return is what sumo_create computes.  A scene that fails a later stage still reports the
 * earlier ones; a failing stage returns the code and message sumo_create gives.
 * development: the Layout as ints in declaration order (returns the count) / the model's and the derived tables' integer members
 * (returns the model count | the Aux count << 16); tools/gen_static_layout.py writes csrc/layout_static.h from them */
int sumo_debug_layout(const void* model_blob, size_t nbytes, int32_t* out, int cap);
int sumo_debug_model_ints(const void* model_blob, size_t nbytes, int32_t* out, int cap, int32_t* aux_out, int aux_cap);
/* development / tests: the two packed role words of each of the 64 lanes, out[2 * lane] and out[2 * lane + 1]
 * (cap >= 128) -- the small integers of a lane's body, dof and joint roles that the kernels keep in registers (bit fields: ROLE0_* /
 * ROLE1_* in csrc/sumo_engine.hip; tests/test_lane_roles_cpu.py unpacks them).  Returns 128, or the error sumo_create gives for a scene
 * in which a value does not fit its field. */
int sumo_debug_lane_roles(const void* model_blob, size_t nbytes, uint32_t* out, int cap);
/* development / tests, host only: the Newton loop's gradient test `scale * sqrt(gn) < tol` as a threshold on gn, the squared gradient
 * norm -- *out = the largest double G with scale * sqrt(G) < tol, so that the test is gn <= G (-1 where no gn >= 0 passes); found by
 * bisection over the bit patterns with IEEE sqrt.  sumo_create computes it once per scene from the model's options. */
int sumo_debug_grad_threshold(double scale, double tol, double* out);
/* development / tests: one wave over caller-given lanes through the in-wave primitives of the engine kernels (all HOST pointers).
 * in64x8 float64 [8][64], int_in64 int32 [64] ->
 *   sums20 float64 [20]: the single wave sum of rows 0 .. 7, then the paired form on rows 0 .. 1, the 4-fold on rows 0 .. 3 and the
 *                        6-fold on rows 0 .. 5;
 *   swapped64 float64 [64]: row 0 exchanged between neighbouring lanes (lane i receives lane i ^ 1);
 *   scan65 int32 [65]: the exclusive scan of int_in64 and, last, its total;
 *   grad_out uint8 [ngn][2]: for each gn[i] the gradient test in its sqrt form (scale * sqrt(gn) < tol, evaluated on the device) and in
 *                        its threshold form (gn <= sumo_debug_grad_threshold(scale, tol)).  ngn may be 0. */
int sumo_debug_wave_ops(sumo_handle_t h, const double* in64x8, const int32_t* int_in64, double* sums20, double* swapped64,
                        int32_t* scan65, const double* gn, int ngn, double scale, double tol, uint8_t* grad_out);
/* development (-DSUMO_DBG_DUMP builds): device buffer [20][8][64] float64 that receives intermediate vectors of env 0's forward
 * evaluations (tools/dump_diff.py); NULL = off */
int sumo_debug_dump(sumo_handle_t h, double* dev_buf);
/* development / tests: the first hand-over of env `env` in the following fused launches carries a wrong checksum (-1 = off) */
int sumo_debug_fault(sumo_handle_t h, int env);
/* device-side statistics accumulated since creation: forward calls, newton iterations, contacts, efc rows,
 * max ncon, max nefc, max newton iterations, dropped contacts, diverged env steps, aborted waits of the fused rollout's step
 * hand-over, hand-over tag / checksum mismatches (both always 0 unless a launch was cut short); contact-generation fidelity
 * accounting, SAMPLED in the forward evaluation that opens each env step (1 in 20 forwards): capsule-box calls that yielded 3 active contacts (MuJoCo's mjc_CapsuleBox yields at most 2), active contacts on a
 * border rod beyond the cylinder's flat end (the rods collide as capsules of the same radius / half length: the only place where
 * the shape differs from MuJoCo's cylinder) (HOST float64 [SUMO_NSTATS]). */
#define SUMO_NSTATS 13
int sumo_stats(sumo_handle_t h, double* out);
/* per-phase shader-cycle totals (20 phases + 4 ad-hoc probe slots); all zero unless the library was built with
 * -DSUMO_PROFILE (HOST float64 [24]). */
int sumo_profile(sumo_handle_t h, double* out24);

/* development: from the next sumo_step on, every env wave stores {start stamp, end stamp (100 MHz s_memrealtime),
 * Newton iterations | contacts << 32, dense-solver forwards | constraint rows << 32} of its step in stamps_dev (DEVICE
 * uint64 [E][4]); NULL switches the trace off.  Used by tools/slot_trace.py. */
int sumo_debug_trace(sumo_handle_t h, uint64_t* stamps_dev);

#ifdef __cplusplus
}
#endif
#endif
