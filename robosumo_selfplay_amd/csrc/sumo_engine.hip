// sumo_engine.hip -- MI355X (gfx950) batched RoboSumo environment engine: kernels + C ABI (include/sumo_hip.h).
//
// One environment per 64-lane wavefront (one wave per workgroup).  The whole env step -- frame_skip x RK4 x
// forward dynamics (kinematics, CoM/CRB mass matrix, collision, pyramidal contact + joint-limit rows, bias forces,
// primal Newton solve), game rules, rewards, done, auto-reset with a counter RNG, observation write -- runs in ONE
// launch; per-env state (qpos, qvel, warm start) is read from / written to HBM once per env step as a contiguous
// record, everything else lives in LDS.  float64 throughout (the reference's mjtNum is double,
// mujoco-py/mujoco_py/pxd/mjmodel.pxd:81).
//
// Reference behaviour being reproduced (file:line are in the reference checkout):
//   env step + auto-reset     subproc_vec_env.py:10-16, sumo_env.py:40-72, robosumo/robosumo/envs/sumo.py:120-202
//   observation               robosumo/robosumo/envs/agents.py:190-214
//   reset                     robosumo/robosumo/envs/sumo.py:232-253, mujoco_env.py:104-119
//   physics                   mujoco_env.py:125-129 -> mjsim.pyx:115-129 -> mj_step (MuJoCo 2.1)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "../../include/sumo_hip.h"
#include "../../include/sumo_model.h"
#include "../../include/sumo_ppo.h"   /* ppo_lstm_net: the recurrent nets of the fused rollout */
#ifdef SUMO_POLICY_PROBE   /* development build: time inside the policy trunks, summed over all waves (sumo_debug_tprobe) */
__device__ unsigned long long g_tprobe[8];
#define PT_PROBE_INIT() unsigned long long tpl_ = __builtin_amdgcn_s_memrealtime()
#define PT_PROBE(k) do { if (lane == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memrealtime(); atomicAdd(&g_tprobe[k], t_ - tpl_); tpl_ = t_; } } while (0)
#endif
#include "ppo_tile.h"   /* MLP(64,64) trunk / Gaussian head on one MFMA tile: the policy phase of the fused rollout kernel */

#define WAVE 64
#ifndef SUMO_WPE
#define SUMO_WPE 2  /* waves per SIMD the register allocator targets: 2 -> at most 256 registers per lane */
#endif
/* Scenes whose LDS footprint leaves (almost) one wave per SIMD anyway -- nv >= 36: 29-38 KB per env, 4-5 waves per CU -- use
 * the whole 512-entry register file of the lane instead of spilling at 256: scratch 648-792 -> 8 B per lane, Spider-vs-Spider
 * 598 -> 858 k env-steps/s, Ant-vs-Spider 727 -> 946 k, Bug-vs-Bug 512 -> 554 k (measured; nv = 32 with 6 waves per CU is
 * faster at two waves per SIMD: 1.21 M against 1.02 M). */
#define SUMO_WPE_OF(nv) ((nv) >= 36 ? 1 : SUMO_WPE)
#define MINVAL 1e-15
#ifndef SUMO_STAT_LDS
#define SUMO_STAT_LDS 0
#endif
#define MAXCHAIN 8   /* dofs on the path root -> body (free joint 6 + hip + ankle) */
#define MAXBCHAIN 4  /* bodies on the path root -> body */
#define PI_D 3.14159265358979323846
#define RNG_NORMAL_BASE 64

// ---------------------------------------------------------------------------------------------------------
// device-side model view
// ---------------------------------------------------------------------------------------------------------
struct Aux {  // derived integer tables (built on the host in build_aux)
  const int* ai;
  const double* af;
  const signed char* pic;  // pos_in_chain[nbody][nv]: slot of dof in the body's chain, -1 if absent
  int ndepth;              // levels 0..ndepth-1 (world = level 0)
  int ntri;                // nv*(nv+1)/2
  int o_lvl_adr, o_lvl_body, o_child_adr, o_child, o_chain_len, o_chain, o_bchain_len, o_bchain, o_body_agent,
      o_tri_i, o_tri_j, o_ent;
  int o_wgmat;  // double table: 9 per geom (valid for world geoms)
  int o_stat_d, n_stat_d, o_stat_i, n_stat_i;  // tables copied into LDS at kernel start (see build_aux)
  int o_wpa;                                   // double table: world geom positions [3*nworld] | axes [3*nworld]
  int nc, nworld;  // collision centres: bodies 0..nbody-1, then one per world geom
  int maxchild;               // largest number of children of any body
  int nstub;                  // jointless leaf bodies whose inertia is merged into their (effective) parent
  int nwp, wrounds, arounds;  // pairs with a static world geom (listed first), rounds of 64 for them / for the rest
};

#define AUX_NINTS ((int)((offsetof(Aux, arounds) + sizeof(int) - offsetof(Aux, ndepth)) / sizeof(int)))   /* the int members: ndepth .. arounds */

struct Layout {  // LDS offsets in doubles unless noted
  int ld;        // leading dimension of H (odd)
  int mld, msize, d1;  // mass matrix: one dense block per agent tree, leading dim mld (odd); d1 = first dof of agent 1
  int maxcon, maxefc, maxcand;
  int jbcap;     // capacity of the contact-Jacobian pool in 24-double halves (3 rows x 8 slots); a contact between two
                 // moving bodies takes two halves, a contact with the world one
  int tree_ok;    // the dof tree has the shape tree_factor_solve assumes (checked in build_layout)
  int force_dense;  // development (SUMO_FORCE_DENSE_H=1): Newton Hessians always through the general dense path
  int warm_mode;  // 0: MuJoCo semantics (solver starts from qacc_warmstart of the previous mj_step); 1: RK stages 2-4 start
                  // from the previous stage's solution (same optimum within the solver tolerance, fewer Newton iterations)
  int qpos, qvel, warm, ctrl, x0, accv, acca, tmpv;
  int xpos, xquat, xipos, gaxis, xanchor, xaxis, com, cinert, cdof, abuf, cfrc;  // "kin scratch"
  int H;                                                                           // aliases kin scratch
  int M, bias, qsm, asmo, Ma, grad, search, Mv, x, dlim;
  int stash;     // 4 doubles parked across the step loop (+ 8 for the fused rollout: ticket, reward inputs, episode record, development clock)
  int cmask;     // per dof: 64-bit mask of the contacts whose Jacobian touches the dof
  int cond, Jb, cpar, cW, cp, jar, D, aref;
  int limD, limA;  // joint-limit slots, hinge-indexed: [nhinge] lower side | [nhinge] upper side (D = 0: side not active)
  int nhinge;
  int stat_d;    // static double tables: csize[2*nc] | cinvw[nc] | wbox[12*nworld] | wlim[6*nworld]
  int i_base;  // start of int region (in doubles)
  // int region offsets (in ints, relative to int base)
  int con_b;
  int b_dofidx;  // byte offset (relative to int base): signed char [16 * maxcon], dof of each Jacobian slot or -1
  int stat_i;    // static int tables: ctype[nc] | cbody[nc] | chain[2*nbody] | chlen_agent[nbody]
  int total_bytes;
};

// Compile-time copy of the Layout of the flagship scene (Ant-vs-Ant, default settings), generated by tools/gen_static_layout.py from
// build_layout() itself (sumo_debug_layout).  With it every `c.L.field` of the hot kernels is an immediate: LDS addresses become
// `lane-dependent base + constant offset` (one shift per lane index instead of an add per array), and the ~60 wave-uniform words of
// the runtime Layout no longer compete for the 102 SGPRs.  sumo_create compares the scene's runtime Layout with this table word
// for word and uses the static kernel variants only on an exact match (any other scene / setting: the runtime-Layout variants).
#include "layout_static.h"

struct StepArgs {
  double* state;       // [N][state_stride]
  int* counters;       // [N][4] num_steps, reset_count, -, -
  uint64_t* seeds;     // [N]
  int state_stride;
  const float* actions;
  float* obs;
  double* info;
  uint8_t* done;
  double* ep_r;
  double* ep_dr;
  int* ep_l;
  const uint8_t* mask;  // reset only
  const int* perm;      // step: workgroup b advances env perm[b] (NULL = identity); see sumo_step
  int* cost;            // step: per-env work estimate written for the next launch's schedule
  const int* rank_cost; // step: the first rank_blocks workgroups rank these estimates (of the previous launch) into
  int* rank_perm;       //       the schedule of the NEXT launch instead of advancing an env (sched_rank)
  int rank_blocks;
  unsigned long long* trace;   // development: [N][4] wall-clock (100 MHz) stamps of each env wave's start / end, work counters (sumo_debug_trace)
  unsigned long long* stats;
  int obs_stride, act_stride;
  int N;
  // fused rollout (sumo_rollout_kernel): hand-over tag of this launch (tag of an env after its k-th step = seq_base + k), the
  // launch's abort flag, development fault injection (env whose first hand-over carries a wrong checksum; -1 = off)
  int seq_base;
  int* abort_flag;
  int dbg_fault_env;
  // debug forward
  const double* dbg_ctrl;
  double* dbg_qacc;
  int* dbg_counts;
};

#define MI(name) (pt_global(mdl.ibase) + mdl.o_##name)
#define MF(name) (pt_global(mdl.fbase) + mdl.o_##name)
#define AI(name) (pt_global(aux.ai) + aux.o_##name)

/* One wavefront per workgroup: LDS operations of a wave are issued and completed in order, so phases only need a
 * compiler barrier between them (no s_waitcnt drain of unrelated loads, no s_barrier). */
#define SYNC() asm volatile("" ::: "memory")

// ---------------------------------------------------------------------------------------------------------
// small math
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double fast_rcp(double x) {  // v_rcp_f64 + two Newton steps (~1 ulp)
  double r = __builtin_amdgcn_rcp(x);
  r = r * (2.0 - x * r);
  r = r * (2.0 - x * r);
  return r;
}
__device__ __forceinline__ double fast_rsqrt(double x) {  // v_rsq_f64 + two Newton steps (~1 ulp)
  double r = __builtin_amdgcn_rsq(x);
  r = r * (1.5 - 0.5 * x * r * r);
  r = r * (1.5 - 0.5 * x * r * r);
  return r;
}
__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void cross3(double* r, const double* a, const double* b) {
  double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  r[0] = x; r[1] = y; r[2] = z;
}
__device__ __forceinline__ double normalize3(double* v) {
  double s = dot3(v, v);
  if (s < MINVAL * MINVAL) { v[0] = 1; v[1] = 0; v[2] = 0; return sqrt(s); }
  double r = fast_rsqrt(s);
  v[0] *= r; v[1] *= r; v[2] *= r;
  return s * r;
}
__device__ __forceinline__ void normalize4(double* q) {
  double s = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (s < MINVAL * MINVAL) { q[0] = 1; q[1] = q[2] = q[3] = 0; return; }
  double r = fast_rsqrt(s);
  q[0] *= r; q[1] *= r; q[2] *= r; q[3] *= r;
}
__device__ __forceinline__ void mulquat(double* r, const double* a, const double* b) {
  double t0 = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  double t1 = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  double t2 = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  double t3 = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = t0; r[1] = t1; r[2] = t2; r[3] = t3;
}
__device__ __forceinline__ void quat2mat(double* m, const double* q) {
  double w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}
__device__ __forceinline__ void mulmatvec3(double* r, const double* m, const double* v) {
  double x = m[0] * v[0] + m[1] * v[1] + m[2] * v[2], y = m[3] * v[0] + m[4] * v[1] + m[5] * v[2],
         z = m[6] * v[0] + m[7] * v[1] + m[8] * v[2];
  r[0] = x; r[1] = y; r[2] = z;
}
__device__ __forceinline__ void mulmatTvec3(double* r, const double* m, const double* v) {
  double x = m[0] * v[0] + m[3] * v[1] + m[6] * v[2], y = m[1] * v[0] + m[4] * v[1] + m[7] * v[2],
         z = m[2] * v[0] + m[5] * v[1] + m[8] * v[2];
  r[0] = x; r[1] = y; r[2] = z;
}
// Library transcendentals used once per env step (reset draws, push reward) are called out of line: inlined, their
// coefficient tables are materialised in the kernel prologue and then live in registers / scratch through all twenty
// forward-dynamics evaluations.
__device__ __noinline__ double slow_sin(double x) { return sin(x); }
__device__ __noinline__ double slow_cos(double x) { return cos(x); }
__device__ __noinline__ double slow_log(double x) { return log(x); }
__device__ __noinline__ double slow_exp(double x) { return exp(x); }
// a floating-point constant the compiler cannot hoist (same reason)
#define OPAQUE_F64(name, val)                                                                                        \
  double name;                                                                                                       \
  {                                                                                                                  \
    int lo_, hi_;                                                                                                    \
    asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3"                                                              \
                 : "=v"(lo_), "=v"(hi_)                                                                              \
                 : "i"((int)(__builtin_bit_cast(unsigned long long, (double)(val)) & 0xFFFFFFFFull)),                \
                   "i"((int)(__builtin_bit_cast(unsigned long long, (double)(val)) >> 32)));                         \
    name = __hiloint2double(hi_, lo_);                                                                               \
  }
// sin / cos to ~1 ulp for |x| < 1e6 (Cody-Waite reduction by pi/2 + the fdlibm kernel polynomials); the library routine,
// whose argument reduction dominates its cost, only for larger arguments
__device__ __forceinline__ void fast_sincos(double x, double* sn, double* cs) {
  if (fabs(x) > 1e6) { *sn = slow_sin(x); *cs = slow_cos(x); return; }   // (two-term reduction is exact below ~1.6e6)
  const double fn = rint(x * 6.36619772367581382433e-01);
  double r = fma(-fn, 1.57079632673412561417e+00, x);
  r = fma(-fn, 6.07710050650619224932e-11, r);
  const double z = r * r;
  // (coefficients are rematerialised at each call: hoisted out of the step loop they would sit in registers / scratch for
  // the whole launch)
#define SC_K(name, val) OPAQUE_F64(name, val)
  SC_K(S1, -1.66666666666666324348e-01); SC_K(S2, 8.33333333332248946124e-03); SC_K(S3, -1.98412698298579493134e-04);
  SC_K(S4, 2.75573137070700676789e-06); SC_K(S5, -2.50507602534068634195e-08); SC_K(S6, 1.58969099521155010221e-10);
  SC_K(C1, 4.16666666666666019037e-02); SC_K(C2, -1.38888888888741095749e-03); SC_K(C3, 2.48015872894767294178e-05);
  SC_K(C4, -2.75573143513906633035e-07); SC_K(C5, 2.08757232129817482790e-09); SC_K(C6, -1.13596475577881948265e-11);
#undef SC_K
  const double ps = r + r * z * (S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))));
  const double pc = 1.0 - 0.5 * z + z * z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
  const int q = (int)fn & 3;
  const double s0 = (q & 1) ? pc : ps, c0 = (q & 1) ? ps : pc;
  *sn = (q & 2) ? -s0 : s0;
  *cs = ((q + 1) & 2) ? -c0 : c0;
}
__device__ __forceinline__ void axisangle2quat(double* q, const double* axis, double angle) {
  double s, cs;
  fast_sincos(angle * 0.5, &s, &cs);
  q[0] = cs; q[1] = axis[0] * s; q[2] = axis[1] * s; q[3] = axis[2] * s;
}
__device__ __forceinline__ double dot6(const double* a, const double* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
}
__device__ __forceinline__ void mul_inert_vec(double* r, const double* i, const double* v) {
  r[0] = i[0] * v[0] + i[3] * v[1] + i[4] * v[2] - i[8] * v[4] + i[7] * v[5];
  r[1] = i[3] * v[0] + i[1] * v[1] + i[5] * v[2] + i[8] * v[3] - i[6] * v[5];
  r[2] = i[4] * v[0] + i[5] * v[1] + i[2] * v[2] - i[7] * v[3] + i[6] * v[4];
  r[3] = i[8] * v[1] - i[7] * v[2] + i[9] * v[3];
  r[4] = i[6] * v[2] - i[8] * v[0] + i[9] * v[4];
  r[5] = i[7] * v[0] - i[6] * v[1] + i[9] * v[5];
}
__device__ __forceinline__ void cross_motion(double* r, const double* vel, const double* v) {
  r[0] = -vel[2] * v[1] + vel[1] * v[2];
  r[1] = vel[2] * v[0] - vel[0] * v[2];
  r[2] = -vel[1] * v[0] + vel[0] * v[1];
  r[3] = -vel[2] * v[4] + vel[1] * v[5] - vel[5] * v[1] + vel[4] * v[2];
  r[4] = vel[2] * v[3] - vel[0] * v[5] + vel[5] * v[0] - vel[3] * v[2];
  r[5] = -vel[1] * v[3] + vel[0] * v[4] - vel[4] * v[0] + vel[3] * v[1];
}
__device__ __forceinline__ void cross_force(double* r, const double* vel, const double* f) {
  r[0] = -vel[2] * f[1] + vel[1] * f[2] - vel[5] * f[4] + vel[4] * f[5];
  r[1] = vel[2] * f[0] - vel[0] * f[2] + vel[5] * f[3] - vel[3] * f[5];
  r[2] = -vel[1] * f[0] + vel[0] * f[1] - vel[4] * f[3] + vel[3] * f[4];
  r[3] = -vel[2] * f[4] + vel[1] * f[5];
  r[4] = vel[2] * f[3] - vel[0] * f[5];
  r[5] = -vel[1] * f[3] + vel[0] * f[4];
}
// DPP move of a double (two 32-bit halves), every row enabled, bound_ctrl on: a lane without a source reads 0.  (With bound_ctrl
// off the builtin's `old` operand is live, and the compiler fills it with a v_mov 0 in front of every DPP move.)
template <int CTRL>
__device__ __forceinline__ double dpp_mov_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
  int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}
// wave-wide sum, returned wave-uniform from lane 63: in-row scan with row_shr, then row_bcast 15 / 31.  The two broadcast stages
// run with every row enabled: lane 63 takes lane 47 (its row's source) in the first and lane 31 in the second, lane 31 took lane 15
// in the first, and each source is read before its own stage's add -- lane 63 ends as (d63 + d47) + (d31 + d15), d the row totals.
// The lanes of rows 0 and 2 hold other (defined) numbers after these stages; nothing reads a lane but through the readlane of 63.
#define WAVE_SUM_STAGES(X) X(0x111) X(0x112) X(0x114) X(0x118) X(0x142) X(0x143)   /* row_shr 1, 2, 4, 8; row_bcast 15, 31 */
__device__ __forceinline__ double wave_sum(double v) {
#define WAVE_SUM_STAGE(CTRL) v += dpp_mov_f64<CTRL>(v);
  WAVE_SUM_STAGES(WAVE_SUM_STAGE)
#undef WAVE_SUM_STAGE
  return readlane_f64(v, 63);
}
// N wave sums whose inputs are ready together: wave_sum's adds per value, the stages of the chains interleaved
template <int N>
__device__ __forceinline__ void wave_sum_n(double (&v)[N]) {
#define WAVE_SUM_STAGE(CTRL) _Pragma("unroll") for (int k = 0; k < N; k++) v[k] += dpp_mov_f64<CTRL>(v[k]);
  WAVE_SUM_STAGES(WAVE_SUM_STAGE)
#undef WAVE_SUM_STAGE
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = readlane_f64(v[k], 63);
}
__device__ __forceinline__ void wave_sum2(double& a, double& b) {
  double v[2] = {a, b};
  wave_sum_n(v);
  a = v[0]; b = v[1];
}
__device__ __forceinline__ void wave_sum4(double& a, double& b, double& c, double& d) {
  double v[4] = {a, b, c, d};
  wave_sum_n(v);
  a = v[0]; b = v[1]; c = v[2]; d = v[3];
}
// exclusive scan over the wave + total.  Every lane's value is used: the row_shr stages read 0 where there is no source
// (bound_ctrl), the two row_bcast stages keep their row masks and the `old` operand that the masked rows take.
__device__ __forceinline__ int wave_excl_scan(int v, int lane, int* total) {
  int inc = v;
  inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xF, 0xF, true);
  inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xF, 0xF, true);
  inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xF, 0xF, true);
  inc += __builtin_amdgcn_update_dpp(0, inc, 0x118, 0xF, 0xF, true);
  inc += __builtin_amdgcn_update_dpp(0, inc, 0x142, 0xA, 0xF, false);
  inc += __builtin_amdgcn_update_dpp(0, inc, 0x143, 0xC, 0xF, false);
  *total = __builtin_amdgcn_readlane(inc, 63);
  return inc - v;
}

// Contact-generation fidelity accounting, once per forward evaluation and OUT OF LINE (its own register allocation; the hot loops
// of the collision phase are not touched): among the `ncon` contacts just stored (cond [14 per contact]: dist, pos[3], frame[9], -;
// cb [4 per contact]: body1, body2, pair, -) counts
//   * capsule-box calls that produced three active contacts -- three consecutive contacts of one pair (only capsule-box yields
//     three; MuJoCo's mjc_CapsuleBox at most two) -- low 16 bits;
//   * contacts on a border rod (a world CYLINDER, collided as a capsule) that lie beyond the cylinder's flat end, i.e. on the
//     capsule's end cap, the only place where the two shapes differ -- high 16 bits.
__device__ __noinline__ int fidelity_count(const double* cond, const int* cb, int ncon, int lane, const int32_t PT_GAS* pair_geom2,
                                           const int32_t PT_GAS* geom_type, const double PT_GAS* geom_pos, const double PT_GAS* geom_quat,
                                           const double PT_GAS* geom_size) {
  int cb3 = 0, rod = 0;
  if (lane < ncon) {
    const int p = cb[4 * lane + 2];
    if (lane + 2 < ncon && cb[4 * (lane + 1) + 2] == p && cb[4 * (lane + 2) + 2] == p) cb3 = 1;
    if (cb[4 * lane + 1] == 0) {   // the second body is the world
      const int g2 = pair_geom2[p];
      if (geom_type[g2] == SUMO_GEOM_CYLINDER) {
        const double w = geom_quat[4 * g2], x = geom_quat[4 * g2 + 1], y = geom_quat[4 * g2 + 2], z = geom_quat[4 * g2 + 3];
        const double ax[3] = {2 * (x * z + w * y), 2 * (y * z - w * x), w * w - x * x - y * y + z * z};   // the rod's axis: z column of its frame
        const double d = (cond[14 * lane + 1] - geom_pos[3 * g2]) * ax[0] + (cond[14 * lane + 2] - geom_pos[3 * g2 + 1]) * ax[1] +
                         (cond[14 * lane + 3] - geom_pos[3 * g2 + 2]) * ax[2];
        rod = fabs(d) > geom_size[3 * g2 + 1];
      }
    }
  }
  return __popcll(__ballot(cb3)) | (__popcll(__ballot(rod)) << 16);
}

// ---------------------------------------------------------------------------------------------------------
// narrow phase primitives.  A lane produces up to 3 contacts {dist, pos, normal} in registers.
// ---------------------------------------------------------------------------------------------------------
struct Con1 { double dist, pos[3], nrm[3]; int ok; };

__device__ __forceinline__ void sphere_sphere(Con1& c, double margin, const double* p1, double r1, const double* p2, double r2) {
  double dif[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  double cd2 = dot3(dif, dif), mind = margin + r1 + r2;
  c.ok = 0;
  if (cd2 > mind * mind) return;
  double len;
  if (cd2 < MINVAL * MINVAL) { len = sqrt(cd2); dif[0] = 0; dif[1] = 0; dif[2] = 1; }
  else { double ri = fast_rsqrt(cd2); len = cd2 * ri; dif[0] *= ri; dif[1] *= ri; dif[2] *= ri; }
  c.dist = len - r1 - r2;
  for (int k = 0; k < 3; k++) { c.nrm[k] = dif[k]; c.pos[k] = p1[k] + dif[k] * (r1 + 0.5 * c.dist); }
  c.ok = 1;
}
__device__ __forceinline__ void plane_sphere(Con1& c, double margin, const double* pp, const double* n, const double* sp, double r) {
  double t[3] = {sp[0] - pp[0], sp[1] - pp[1], sp[2] - pp[2]};
  double cd = dot3(t, n);
  c.ok = 0;
  if (cd > margin + r) return;
  c.dist = cd - r;
  for (int k = 0; k < 3; k++) { c.nrm[k] = n[k]; c.pos[k] = sp[k] - n[k] * (r + 0.5 * c.dist); }
  c.ok = 1;
}
__device__ __forceinline__ void sphere_box(Con1& c, double margin, const double* sp, double r, const double* bp, const double* bm,
                                           const double* bs) {
  double t[3] = {sp[0] - bp[0], sp[1] - bp[1], sp[2] - bp[2]}, ctr[3], cl[3], dl[3];
  mulmatTvec3(ctr, bm, t);
  for (int k = 0; k < 3; k++) { cl[k] = ctr[k] > bs[k] ? bs[k] : (ctr[k] < -bs[k] ? -bs[k] : ctr[k]); dl[k] = cl[k] - ctr[k]; }
  const double dd2 = dot3(dl, dl);
  const double idist = dd2 > 0 ? fast_rsqrt(dd2) : 0.0, dist = dd2 * idist;
  c.ok = 0;
  if (dist - r > margin) return;
  double nl[3], pl[3];
  if (dist <= MINVAL) {
    double best = 1e300; int kb = 0, sb = 1;
    for (int k = 0; k < 3; k++)
      for (int s = -1; s <= 1; s += 2) {
        double fd = fabs(s * bs[k] - ctr[k]);
        if (fd < best) { best = fd; kb = k; sb = s; }
      }
    nl[0] = nl[1] = nl[2] = 0;
    if (kb == 0) nl[0] = -sb; else if (kb == 1) nl[1] = -sb; else nl[2] = -sb;
    c.dist = -best - r;
  } else {
    for (int k = 0; k < 3; k++) nl[k] = dl[k] * idist;
    c.dist = dist - r;
  }
  for (int k = 0; k < 3; k++) pl[k] = ctr[k] + nl[k] * (r + 0.5 * c.dist);
  double pw[3];
  mulmatvec3(c.nrm, bm, nl);
  mulmatvec3(pw, bm, pl);
  for (int k = 0; k < 3; k++) c.pos[k] = pw[k] + bp[k];
  c.ok = 1;
}
// `skip`: coordinate that sits exactly on a box face at t (its own breakpoint) and contributes exactly 0
__device__ __forceinline__ double seg_box_dgrad(const double* cc, const double* a, const double* bs, double t, int skip = -1) {
  double g = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (k == skip) continue;
    double p = cc[k] + t * a[k];
    if (p > bs[k]) g += a[k] * (p - bs[k]);
    else if (p < -bs[k]) g += a[k] * (p + bs[k]);
  }
  return g;
}

// ---------------------------------------------------------------------------------------------------------
// the per-wave environment context
// ---------------------------------------------------------------------------------------------------------
// Per-lane constants, loaded into registers once per launch (a lane keeps the same roles -- body `lane`, dof `lane`,
// joint `lane`, actuator `lane`, pair `lane + 64 r` -- for all 20 forward-dynamics evaluations of an env step).
struct LaneRec {
  // body role
  double b_pos[3], b_quat[4], b_ipos[3], b_iquat[4], b_inertia[3], b_mass;
  double j_pos[3], j_axis[3], j_qpos0;      // the body's hinge (bodies carry at most one joint)
  int b_parent, b_level, b_agent, b_isfree, b_jnt, b_qadr, b_nchild, b_bchain_len, b_chain_len;
  unsigned long long b_child;               // child body ids, one per byte, descending
  unsigned b_bchain;                        // body ids root -> self, one per byte
  unsigned long long b_chain;               // dof ids root -> body, one per byte
  unsigned b_chain_own, b_chain_free;       // bit p: chain[p] belongs to this body / starts a free joint
  // inertial constants used for cinert: the body's own, or -- when jointless leaf bodies are rigidly attached to it -- those of
  // the merged rigid body; body frame, inertia about the (merged) centre of mass as xx yy zz xy xz yz; zero for the leaves
  double c_I[6], c_ipos[3], c_mass;
  // dof role
  double d_arm, d_damp;
  int d_body, d_pos;                        // d_pos: position of the dof in d_chain
  unsigned long long d_chain;               // chain of the dof's body
  // joint role
  double jt_lo, jt_hi, jt_margin, jt_invw;
  int jt_type, jt_qadr, jt_dadr, jt_limited, jt_body, jt_agent;
  int jt_hid, d_hid;                        // running index of the hinge (joint role / dof role), -1 for free-joint dofs
  // actuator role
  double a_gear, a_lo, a_hi;
  int a_dof, pad_;
  // the lane's small integers of all roles, packed (build_lane_roles; ROLE0_* / ROLE1_* below): read once per launch into Ctx
  unsigned role0, role1;
};
// Bit fields of the two role words, {first bit, width}.  A lane keeps them in two registers for the whole launch, so the address
// arithmetic and the branches of a phase do not wait for the constant record: what a phase still reads from the record (its doubles,
// the chain bytes) travels while the LDS reads are already in flight.  build_lane_roles refuses a scene whose field does not fit.
//   role0  body role: level + 1 (0: lane is no body), agent, joint is free, joint is a hinge, parent, number of children, lengths of
//          the dof chain and of the body chain, qpos address of the joint; joint role: is a hinge, limited, agent
//   role1  dof role: hinge index + 1 (0: none), position in its body's dof chain, body; joint role: free joints before it (from
//          which dof address = j + 5 f, qpos address = j + 6 f, hinge index = j - f follow: free joints carry 6 dofs / 7 qpos,
//          hinges 1 / 1), body; body role: last dof of its chain
#define ROLE0_LEVEL1 0, 3
#define ROLE0_AGENT 3, 1
#define ROLE0_ISFREE 4, 1
#define ROLE0_HINGE 5, 1
#define ROLE0_PARENT 6, 6
#define ROLE0_NCHILD 12, 4
#define ROLE0_CHAIN_LEN 16, 4
#define ROLE0_BCHAIN_LEN 20, 3
#define ROLE0_QADR 23, 6
#define ROLE0_JT_HINGE 29, 1
#define ROLE0_JT_LIMITED 30, 1
#define ROLE0_JT_AGENT 31, 1
#define ROLE1_HID1 0, 6
#define ROLE1_DPOS 6, 4
#define ROLE1_DBODY 10, 6
#define ROLE1_JT_NFREE 16, 2
#define ROLE1_JT_BODY 18, 6
#define ROLE1_LDOF 24, 6
__host__ __device__ __forceinline__ int role_bits(unsigned w, int lo, int n) { return (int)((w >> lo) & ((1u << n) - 1u)); }

struct Params {  // lives in device memory; read through scalar / per-lane loads
  sumo_model_t mdl; Aux aux; Layout L;
  const LaneRec* lanes;     // [64]
  const int* pair_rec;      // [(wrounds + arounds) * 64] packed pair records (see build_aux)
  const float* pair_bound;  // conservative (rounded-up) reach of each pair
  double adjust_z;          // Agent._adjust_z (agents.py:33,155-161): added to the z an agent REPORTS -- observations and lose test; 0 in training
  double grad_thresh;       // newton_solve's gradient test as a threshold on the squared norm (grad_threshold)
};

template <int NV_, class LT_ = Layout>
struct Ctx {
  typedef LT_ LT;
  static constexpr int NV = NV_;                                  // compile-time nv (register-resident factorisation)
  static constexpr int EPL = (NV_ * (NV_ + 1) / 2 + WAVE - 1) / WAVE;
  LT L;                 // LDS layout: the runtime Layout copied from Params once per launch (wave-uniform -> SGPRs), or the static table
  const LaneRec* kp;    // this lane's constant record (device memory, L1-resident); phases copy the fields they need
  const int* prp;       // this lane's packed pair records / bounds: element r*64
  const float* pbp;
  const Params* P;
  double* sm;    // LDS base (doubles)
  int* si;       // LDS int region
  unsigned char* sb;  // LDS byte region (slotof)
  int lane;
  unsigned role0, role1;   // this lane's packed integer roles (LaneRec::role0 / role1), read through the role_*() accessors
  // per-forward scalars (wave-uniform)
  int ncon, nlim, nefc, ndropped, use_prev, htree;  // htree: every contact has one moving body -> H is tree-sparse like M
#ifdef SUMO_PROFILE
  long long tprev;
  unsigned long long prof[24];   // 20 phases + 4 ad-hoc probe slots (PROBE(k))
#endif
  // statistics accumulated over the launch
  int st_forward, st_newton, st_ncon, st_nefc, st_maxcon, st_maxefc, st_maxnewton, st_dropped, st_dense, st_cross;
  int st_diverged;   // env steps of this launch whose state failed MuJoCo's bad-value test (state_is_bad)
  // contact-generation fidelity accounting (deviations 1-2): capsule-box calls that produced 3 active contacts (MuJoCo's
  // mjc_CapsuleBox gives at most 2) and active contacts on a border rod that lie beyond the cylinder's flat end (the rods collide
  // as capsules: only there does the shape differ from MuJoCo's cylinder)
  int st_cb3, st_rodcap;
  int hcross;
#ifdef SUMO_DBG_DUMP
  double* dbg;   // development: intermediate vectors of env 0's first two forward evaluations (sumo_debug_dump)
#endif
};

// The model / aux views of a context: the runtime structs in device memory, or -- static-Layout variants -- objects whose integer
// members are compile-time constants of the flagship scene (layout_static.h) and whose three pointers are read from Params.
template <class C>
__device__ __forceinline__ decltype(auto) model_view(const C& c) {
  if constexpr (std::is_same<typename C::LT, Layout>::value) return (const sumo_model_t&)c.P->mdl;
  else { typename C::LT::Model m; m.ibase = c.P->mdl.ibase; m.fbase = c.P->mdl.fbase; m.tatami_size = c.P->mdl.tatami_size; return m; }
}
template <class C>
__device__ __forceinline__ decltype(auto) aux_view(const C& c) {
  if constexpr (std::is_same<typename C::LT, Layout>::value) return (const Aux&)c.P->aux;
  else { typename C::LT::AuxT x; x.ai = c.P->aux.ai; x.af = c.P->aux.af; x.pic = c.P->aux.pic; return x; }
}
#define S(off) (c.sm + c.L.off)
// Per-lane constants are re-read at the start of each phase instead of being pinned in registers for the whole launch
// (the optimisation barrier stops the compiler from hoisting the loads back to kernel entry): this keeps the kernel
// within 256 registers, i.e. two waves per SIMD.
template <class T>
__device__ __forceinline__ const T* launder_ptr(const T* p) { asm volatile("" : "+v"(p)); return p; }
template <class PTR>
__device__ __forceinline__ PTR launder_sptr(PTR p) { asm volatile("" : "+s"(p)); return p; }   // wave-uniform pointer (SGPR pair), any address space
// a record of a constant table, read through a global-address-space pointer dword by dword (only the fields that are used
// survive; a laundered pointer is a generic one, whose flat loads would occupy the LDS counter too -- see PT_GAS in ppo_tile.h)
template <class T>
__device__ __forceinline__ T load_rec(const T* p) {
  static_assert(sizeof(T) % 4 == 0, "whole dwords");
  T out;
  const uint32_t PT_GAS* s_ = (const uint32_t PT_GAS*)p;
  uint32_t* d_ = (uint32_t*)&out;
#pragma unroll
  for (unsigned i_ = 0; i_ < sizeof(T) / 4; i_++) d_[i_] = s_[i_];
  return out;
}
#define KCONSTS() const LaneRec K = load_rec(launder_ptr(c.kp))
// the lane's integer roles, from the two role words in registers (no memory access)
// The word is made opaque at every use: the words are loop invariant, and fields the compiler may extract once would each occupy a
// register of their own for the whole launch -- the budget that the per-phase record reads and the opaque lane id protect.
__device__ __forceinline__ int role_get(unsigned w, int lo, int n) { asm volatile("" : "+v"(w)); return role_bits(w, lo, n); }
template <class C> __device__ __forceinline__ int role_level(const C& c) { return role_get(c.role0, ROLE0_LEVEL1) - 1; }
template <class C> __device__ __forceinline__ int role_agent(const C& c) { return role_get(c.role0, ROLE0_AGENT); }
template <class C> __device__ __forceinline__ bool role_isfree(const C& c) { return role_get(c.role0, ROLE0_ISFREE) != 0; }
template <class C> __device__ __forceinline__ bool role_hinge(const C& c) { return role_get(c.role0, ROLE0_HINGE) != 0; }   // the body's joint is a hinge
template <class C> __device__ __forceinline__ int role_parent(const C& c) { return role_get(c.role0, ROLE0_PARENT); }
template <class C> __device__ __forceinline__ int role_nchild(const C& c) { return role_get(c.role0, ROLE0_NCHILD); }
template <class C> __device__ __forceinline__ int role_chain_len(const C& c) { return role_get(c.role0, ROLE0_CHAIN_LEN); }
template <class C> __device__ __forceinline__ int role_bchain_len(const C& c) { return role_get(c.role0, ROLE0_BCHAIN_LEN); }
template <class C> __device__ __forceinline__ int role_qadr(const C& c) { return role_get(c.role0, ROLE0_QADR); }
template <class C> __device__ __forceinline__ int role_ldof(const C& c) { return role_get(c.role1, ROLE1_LDOF); }
template <class C> __device__ __forceinline__ int role_d_hid(const C& c) { return role_get(c.role1, ROLE1_HID1) - 1; }   // -1: free-joint dof, lane past nv
template <class C> __device__ __forceinline__ int role_d_pos(const C& c) { return role_get(c.role1, ROLE1_DPOS); }
template <class C> __device__ __forceinline__ int role_d_body(const C& c) { return role_get(c.role1, ROLE1_DBODY); }
template <class C> __device__ __forceinline__ bool role_jt_hinge(const C& c) { return role_get(c.role0, ROLE0_JT_HINGE) != 0; }   // else a free joint
template <class C> __device__ __forceinline__ bool role_jt_limited(const C& c) { return role_get(c.role0, ROLE0_JT_LIMITED) != 0; }
template <class C> __device__ __forceinline__ int role_jt_agent(const C& c) { return role_get(c.role0, ROLE0_JT_AGENT); }
template <class C> __device__ __forceinline__ int role_jt_body(const C& c) { return role_get(c.role1, ROLE1_JT_BODY); }
template <class C> __device__ __forceinline__ int role_jt_dadr(const C& c) { return c.lane + 5 * role_get(c.role1, ROLE1_JT_NFREE); }
template <class C> __device__ __forceinline__ int role_jt_qadr(const C& c) { return c.lane + 6 * role_get(c.role1, ROLE1_JT_NFREE); }
template <class C> __device__ __forceinline__ int role_jt_hid(const C& c) { return c.lane - role_get(c.role1, ROLE1_JT_NFREE); }
// mass matrix element (i, j) of the block-diagonal storage; valid when i and j belong to the same agent tree
#define MIDX(i, j) ((i) * c.L.mld + ((j) >= c.L.d1 ? (j) - c.L.d1 : (j)))
#define SAME_TREE(i, j) (((i) >= c.L.d1) == ((j) >= c.L.d1))
#define HP(i, k) ((i) * ((i) + 1) / 2 + (k))  /* packed lower-triangular index, i >= k */
#ifdef SUMO_PROFILE
#define PROF(k) do { long long _t = clock64(); c.prof[k] += (unsigned long long)(_t - c.tprev); c.tprev = _t; } while (0)
#else
#define PROF(k) do { } while (0)
#endif
#define PROBE(k) PROF(20 + (k))   /* development: split a phase; the time up to the probe goes to slot 20+k */

// ---- position / velocity stage --------------------------------------------------------------------------
#define BYTE_OF(word64, p) ((int)(((word64) >> (8 * (p))) & 0xFFull))

// One body's frame from its parent's (mj_kinematics, one tree level per call; lane == body id).  Only what the CHILDREN wait for is
// computed here: the joint's own rotation `ql` (a sin / cos pair that depends on qpos alone) comes from a pass over all bodies before
// the level loop, and the inertial-frame outputs (xipos, gaxis) are left to kin_inertial_frames after it -- the same operations on the
// same operands, but once on all body lanes instead of once per level on 2 - 8 of them.
template <class C>
__device__ __forceinline__ void kin_own_body(C& c, const double (&ql)[4]) {
  KCONSTS();
  const int b = c.lane, pid = K.b_parent;
  double* qpos = S(qpos);
  double xp[3], xq[4], R[9], v[3];
  if (K.b_isfree) {
    double* q = qpos + K.b_qadr;
    double qq[4] = {q[3], q[4], q[5], q[6]};
    normalize4(qq);
    q[3] = qq[0]; q[4] = qq[1]; q[5] = qq[2]; q[6] = qq[3];  // in-place normalisation, as mj_kinematics
    xp[0] = q[0]; xp[1] = q[1]; xp[2] = q[2];
    xq[0] = qq[0]; xq[1] = qq[1]; xq[2] = qq[2]; xq[3] = qq[3];
    for (int k = 0; k < 3; k++) S(xanchor)[3 * K.b_jnt + k] = xp[k];
  } else {
    quat2mat(R, S(xquat) + 4 * pid);
    mulmatvec3(v, R, K.b_pos);
    for (int k = 0; k < 3; k++) xp[k] = S(xpos)[3 * pid + k] + v[k];
    mulquat(xq, S(xquat) + 4 * pid, K.b_quat);
    if (K.b_jnt >= 0) {
      const int j = K.b_jnt;
      double anchor[3];
      quat2mat(R, xq);
      mulmatvec3(v, R, K.j_pos);
      for (int k = 0; k < 3; k++) { anchor[k] = xp[k] + v[k]; S(xanchor)[3 * j + k] = anchor[k]; }
      mulmatvec3(v, R, K.j_axis);
      for (int k = 0; k < 3; k++) S(xaxis)[3 * j + k] = v[k];
      mulquat(xq, xq, ql);
      quat2mat(R, xq);
      mulmatvec3(v, R, K.j_pos);
      for (int k = 0; k < 3; k++) xp[k] = anchor[k] - v[k];
    }
    normalize4(xq);
  }
  for (int k = 0; k < 3; k++) S(xpos)[3 * b + k] = xp[k];
  for (int k = 0; k < 4; k++) S(xquat)[4 * b + k] = xq[k];
}
template <class C>
__device__ __forceinline__ void kin_joint_rotation(C& c, double (&ql)[4]) {   // every body lane at once, before the level loop
  KCONSTS();
  ql[0] = 1.0; ql[1] = ql[2] = ql[3] = 0.0;
  if (c.lane >= 1 && c.lane < c.P->mdl.nbody && !K.b_isfree && K.b_jnt >= 0) axisangle2quat(ql, K.j_axis, S(qpos)[K.b_qadr] - K.j_qpos0);
}
template <class C>
__device__ __forceinline__ void kin_inertial_frames(C& c) {   // every body lane at once, after the level loop (reads its own frame back)
  KCONSTS();
  const int b = c.lane;
  double xp[3], xq[4], R[9], v[3], qi[4];
  for (int k = 0; k < 3; k++) xp[k] = S(xpos)[3 * b + k];
  for (int k = 0; k < 4; k++) xq[k] = S(xquat)[4 * b + k];
  quat2mat(R, xq);
  mulmatvec3(v, R, K.b_ipos);
  for (int k = 0; k < 3; k++) S(xipos)[3 * b + k] = xp[k] + v[k];
  mulquat(qi, xq, K.b_iquat);
  quat2mat(R, qi);
  S(gaxis)[3 * b] = R[2]; S(gaxis)[3 * b + 1] = R[5]; S(gaxis)[3 * b + 2] = R[8];
}

// gather children into parents, level by level, for an array of W doubles per body (lane == body id).  The sums are
// accumulated in registers with the loads of all (up to 8) children issued together: one LDS round trip per level instead
// of a read-modify-write chain per child.
template <int W, int NCH, class C>
__device__ __forceinline__ void gather_up_n(C& c, double* arr) {
  KCONSTS();   // the child ids (b_child) stay in the record
  const int b = c.lane, level = role_level(c), nchild = role_nchild(c);
  for (int lvl = c.P->aux.ndepth - 2; lvl >= 1; lvl--) {
    if (level == lvl && nchild > 0) {
      double acc[W], ch[NCH][W];
#pragma unroll
      for (int k = 0; k < W; k++) acc[k] = arr[W * b + k];
#pragma unroll
      for (int ci = 0; ci < NCH; ci++) {
        const int cb = BYTE_OF(K.b_child, ci < nchild ? ci : 0);
#pragma unroll
        for (int k = 0; k < W; k++) ch[ci][k] = arr[W * cb + k];
      }
#pragma unroll
      for (int ci = 0; ci < NCH; ci++)
        if (ci < nchild) {
#pragma unroll
          for (int k = 0; k < W; k++) acc[k] += ch[ci][k];
        }
#pragma unroll
      for (int k = 0; k < W; k++) arr[W * b + k] = acc[k];
    }
    SYNC();
  }
}

template <int W, class C>
__device__ __forceinline__ void gather_up(C& c, double* arr) {
  if (c.P->aux.maxchild <= 4) gather_up_n<W, 4>(c, arr);   // Ant torsos carry 4 legs, Bug 6, Spider 8
  else gather_up_n<W, 8>(c, arr);
}

template <class C>
__device__ __forceinline__ void position_velocity(C& c) {
  const auto& mdl = model_view(c);
  const auto& aux = aux_view(c);
  const int lane = c.lane;
  const int nb = mdl.nbody, nv = mdl.nv;
  if (lane == 0) {
    S(xpos)[0] = S(xpos)[1] = S(xpos)[2] = 0;
    S(xquat)[0] = 1; S(xquat)[1] = S(xquat)[2] = S(xquat)[3] = 0;
    for (int k = 0; k < 3; k++) { S(xipos)[k] = 0; S(gaxis)[k] = 0; }
  }
  SYNC();
  PROF(0);
  {
    const int my_level = pt_global(launder_ptr(c.kp))->b_level;
    double ql[4];
    kin_joint_rotation(c, ql);
    for (int lvl = 1; lvl < aux.ndepth; lvl++) {
      if (my_level == lvl) kin_own_body(c, ql);
      SYNC();
    }
    if (my_level >= 1 && my_level < aux.ndepth) kin_inertial_frames(c);
    SYNC();
  }
  PROF(1);
  // subtree CoM of each agent's root
  {
    KCONSTS();
    const bool isb = lane >= 1 && lane < nb;
    double px = 0, py = 0, pz = 0;
    if (isb) { px = K.b_mass * S(xipos)[3 * lane]; py = K.b_mass * S(xipos)[3 * lane + 1]; pz = K.b_mass * S(xipos)[3 * lane + 2]; }
    const int ag = isb ? role_agent(c) : -1;
    // six independent wave sums (x, y, z of both agents), their DPP chains interleaved stage by stage
    double cs[6] = {ag == 0 ? px : 0.0, ag == 0 ? py : 0.0, ag == 0 ? pz : 0.0, ag == 1 ? px : 0.0, ag == 1 ? py : 0.0, ag == 1 ? pz : 0.0};
    wave_sum_n(cs);
    const double s0x = cs[0], s0y = cs[1], s0z = cs[2], s1x = cs[3], s1y = cs[4], s1z = cs[5];
    if (lane < 2) {
      const double istm = fast_rcp(MF(body_subtreemass)[MI(agent_torso)[lane]]);
      S(com)[3 * lane] = (lane ? s1x : s0x) * istm; S(com)[3 * lane + 1] = (lane ? s1y : s0y) * istm; S(com)[3 * lane + 2] = (lane ? s1z : s0z) * istm;
    }
  }
  SYNC();
  // cinert per body, cdof per joint
  if (lane >= 1 && lane < nb) {
    KCONSTS();
    const int b = lane, ag = role_agent(c);
    double R[9], cp[3], dif[3], RI[9], T[6];
    quat2mat(R, S(xquat) + 4 * b);
    mulmatvec3(cp, R, K.c_ipos);
    for (int k = 0; k < 3; k++) dif[k] = S(xpos)[3 * b + k] + cp[k] - S(com)[3 * ag + k];
    // T = R I R^T with I = [xx xy xz; xy yy yz; xz yz zz] in the body frame
    const double Ixx = K.c_I[0], Iyy = K.c_I[1], Izz = K.c_I[2], Ixy = K.c_I[3], Ixz = K.c_I[4], Iyz = K.c_I[5];
    for (int r = 0; r < 3; r++) {
      RI[3 * r] = R[3 * r] * Ixx + R[3 * r + 1] * Ixy + R[3 * r + 2] * Ixz;
      RI[3 * r + 1] = R[3 * r] * Ixy + R[3 * r + 1] * Iyy + R[3 * r + 2] * Iyz;
      RI[3 * r + 2] = R[3 * r] * Ixz + R[3 * r + 1] * Iyz + R[3 * r + 2] * Izz;
    }
    T[0] = RI[0] * R[0] + RI[1] * R[1] + RI[2] * R[2];   // xx
    T[1] = RI[3] * R[3] + RI[4] * R[4] + RI[5] * R[5];   // yy
    T[2] = RI[6] * R[6] + RI[7] * R[7] + RI[8] * R[8];   // zz
    T[3] = RI[0] * R[3] + RI[1] * R[4] + RI[2] * R[5];   // xy
    T[4] = RI[0] * R[6] + RI[1] * R[7] + RI[2] * R[8];   // xz
    T[5] = RI[3] * R[6] + RI[4] * R[7] + RI[5] * R[8];   // yz
    double ms = K.c_mass;
    double* res = S(cinert) + 10 * b;
    res[0] = T[0] + ms * (dif[1] * dif[1] + dif[2] * dif[2]);
    res[1] = T[1] + ms * (dif[0] * dif[0] + dif[2] * dif[2]);
    res[2] = T[2] + ms * (dif[0] * dif[0] + dif[1] * dif[1]);
    res[3] = T[3] - ms * dif[0] * dif[1];
    res[4] = T[4] - ms * dif[0] * dif[2];
    res[5] = T[5] - ms * dif[1] * dif[2];
    res[6] = ms * dif[0]; res[7] = ms * dif[1]; res[8] = ms * dif[2];
    res[9] = ms;
  }
  if (lane < mdl.njnt) {
    const int j = lane, b = role_jt_body(c), da = role_jt_dadr(c), ag = role_jt_agent(c);
    double off[3];
    for (int k = 0; k < 3; k++) off[k] = S(com)[3 * ag + k] - S(xanchor)[3 * j + k];
    if (!role_jt_hinge(c)) {
      double R[9];
      quat2mat(R, S(xquat) + 4 * b);
      for (int k = 0; k < 3; k++) {
        double* cd = S(cdof) + 6 * (da + k);
        cd[0] = cd[1] = cd[2] = cd[3] = cd[4] = cd[5] = 0;
        cd[3 + k] = 1;
      }
      for (int k = 0; k < 3; k++) {
        double ax[3] = {R[k], R[3 + k], R[6 + k]};
        double* cd = S(cdof) + 6 * (da + 3 + k);
        cd[0] = ax[0]; cd[1] = ax[1]; cd[2] = ax[2];
        cross3(cd + 3, ax, off);
      }
    } else {
      double* cd = S(cdof) + 6 * da;
      const double* ax = S(xaxis) + 3 * j;
      cd[0] = ax[0]; cd[1] = ax[1]; cd[2] = ax[2];
      cross3(cd + 3, ax, off);
    }
  }
  SYNC();
  PROF(2);
  // body velocities along each body's dof chain; a_b = sum over the body's own dofs of cdof_dot * qvel
  double cvel[6] = {0, 0, 0, 0, 0, 0};
  if (c.L.tree_ok && lane >= 1 && lane < nb) {
    // every body hangs off a free joint (6 dofs) plus at most two hinges (Layout::tree_ok): fixed shape, all loads of the
    // chain's motion axes issued together instead of one round trip per chain element
    // The chain needs no record read in this shape: its first six dofs are the root's (B .. B + 5), a seventh is the hip and
    // an eighth the ankle below it, i.e. the chain's last dof and the one before it.  A body owns the root dofs if its joint
    // is the free one and the chain's last dof if its joint is a hinge (build_lane_roles checks all of it against the chains).
    const int b = lane, len = role_chain_len(c), ld = role_ldof(c);
    const int B = role_agent(c) ? c.L.d1 : 0, j6 = len > 7 ? ld - 1 : (len > 6 ? ld : B), j7 = len > 7 ? ld : B;
    const bool own_root = role_isfree(c), own_last = role_hinge(c);
    const double* qvel = S(qvel);
    double cd[8][6], qv[8], a[6] = {0, 0, 0, 0, 0, 0}, t[6];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int j = k < 6 ? B + k : (k == 6 ? j6 : j7);
      qv[k] = qvel[j];
#pragma unroll
      for (int q = 0; q < 6; q++) cd[k][q] = S(cdof)[6 * j + q];
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int q = 0; q < 6; q++) cvel[q] += cd[k][q] * qv[k];
    if (own_root) {
#pragma unroll
      for (int k = 3; k < 6; k++) {
        cross_motion(t, cvel, cd[k]);
#pragma unroll
        for (int q = 0; q < 6; q++) a[q] += t[q] * qv[k];
      }
    }
#pragma unroll
    for (int k = 3; k < 6; k++)
#pragma unroll
      for (int q = 0; q < 6; q++) cvel[q] += cd[k][q] * qv[k];
#pragma unroll
    for (int k = 6; k < 8; k++) {
      if (k < len) {
        if (own_last && k == len - 1) {
          cross_motion(t, cvel, cd[k]);
#pragma unroll
          for (int q = 0; q < 6; q++) a[q] += t[q] * qv[k];
        }
#pragma unroll
        for (int q = 0; q < 6; q++) cvel[q] += cd[k][q] * qv[k];
      }
    }
#pragma unroll
    for (int q = 0; q < 6; q++) S(abuf)[6 * b + q] = a[q];
  } else if (lane >= 1 && lane < nb) {
    KCONSTS();
    const int b = lane;
    double a[6] = {0, 0, 0, 0, 0, 0}, cd[6];
    const double* qvel = S(qvel);
    const int len = K.b_chain_len;
    int p = 0;
    while (p < len) {
      const int j = BYTE_OF(K.b_chain, p);
      const bool own = (K.b_chain_own >> p) & 1u;
      if ((K.b_chain_free >> p) & 1u) {
        for (int k = 0; k < 3; k++)
          for (int q = 0; q < 6; q++) cvel[q] += S(cdof)[6 * (j + k) + q] * qvel[j + k];
        if (own)
          for (int k = 3; k < 6; k++) {
            cross_motion(cd, cvel, S(cdof) + 6 * (j + k));
            for (int q = 0; q < 6; q++) a[q] += cd[q] * qvel[j + k];
          }
        for (int k = 3; k < 6; k++)
          for (int q = 0; q < 6; q++) cvel[q] += S(cdof)[6 * (j + k) + q] * qvel[j + k];
        p += 6;
      } else {
        if (own) {
          cross_motion(cd, cvel, S(cdof) + 6 * j);
          for (int q = 0; q < 6; q++) a[q] += cd[q] * qvel[j];
        }
        for (int q = 0; q < 6; q++) cvel[q] += S(cdof)[6 * j + q] * qvel[j];
        p += 1;
      }
    }
    for (int q = 0; q < 6; q++) S(abuf)[6 * b + q] = a[q];
  }
  SYNC();
  // RNE forward: cacc along the body chain, cfrc = I*cacc + cvel x* (I*cvel)
  if (lane < nb) {
    const int b = lane;
    double* f = S(cfrc) + 6 * b;
    if (b == 0) { for (int q = 0; q < 6; q++) f[q] = 0; }
    else {
      KCONSTS();   // the body chain (b_bchain) stays in the record
      const int bclen = role_bchain_len(c);
      const double* g = MF(opt) + SUMO_OPT_GRAVITY;
      double cacc[6] = {0, 0, 0, -g[0], -g[1], -g[2]}, t[6], t1[6];
      double ab[MAXBCHAIN][6];
#pragma unroll
      for (int p = 0; p < MAXBCHAIN; p++) {   // all loads in flight; entries past the chain re-read its first body
        const int kb = (K.b_bchain >> (8 * (p < bclen ? p : 0))) & 0xFFu;
#pragma unroll
        for (int q = 0; q < 6; q++) ab[p][q] = S(abuf)[6 * kb + q];
      }
#pragma unroll
      for (int p = 0; p < MAXBCHAIN; p++)
        if (p < bclen) {
#pragma unroll
          for (int q = 0; q < 6; q++) cacc[q] += ab[p][q];
        }
      mul_inert_vec(f, S(cinert) + 10 * b, cacc);
      mul_inert_vec(t, S(cinert) + 10 * b, cvel);
      cross_force(t1, cvel, t);
      for (int q = 0; q < 6; q++) f[q] += t1[q];
    }
  }
  SYNC();
  gather_up<6>(c, S(cfrc));
  if (lane < nv) S(bias)[lane] = dot6(S(cdof) + 6 * lane, S(cfrc) + 6 * role_d_body(c));
  PROF(3);
}

template <class C>
__device__ __forceinline__ void mass_matrix(C& c) {
  KCONSTS();
  const int lane = c.lane, nv = c.P->mdl.nv;
  // the contact records (dead by now) share the mass matrix's storage: clear it only here
  for (int i = lane; i < c.L.msize; i += WAVE) S(M)[i] = 0.0;
  gather_up<10>(c, S(cinert));  // cinert -> composite rigid body inertia, in place (ends with a SYNC)
  if (c.L.tree_ok && lane < nv) {
    // ancestors of dof i in the fixed shape: the root dofs below it, the leg's hip (for an ankle), itself
    const int i = lane, B = i >= c.L.d1 ? c.L.d1 : 0, il = i - B, nr = il < 6 ? il : 6;
    double ci[6], buf[6], r[7][6];
#pragma unroll
    for (int q = 0; q < 6; q++) ci[q] = S(cdof)[6 * i + q];
#pragma unroll
    for (int k = 0; k < 7; k++) {
      const int j = k < 6 ? B + k : i - 1;            // k == 6: the hip of an ankle dof (unused otherwise)
#pragma unroll
      for (int q = 0; q < 6; q++) r[k][q] = S(cdof)[6 * (j < 0 ? 0 : j) + q];
    }
    mul_inert_vec(buf, S(cinert) + 10 * role_d_body(c), ci);
    double* Mi = S(M) + i * c.L.mld;
    Mi[il] = dot6(ci, buf) + K.d_arm;
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (k < nr) { const double v = dot6(r[k], buf); Mi[k] = v; S(M)[(B + k) * c.L.mld + il] = v; }
    if (il >= 6 && (il & 1)) { const double v = dot6(r[6], buf); Mi[il - 1] = v; S(M)[(i - 1) * c.L.mld + il] = v; }
  } else if (lane < nv) {
    const int i = lane;
    double buf[6];
    mul_inert_vec(buf, S(cinert) + 10 * K.d_body, S(cdof) + 6 * i);
    for (int p = K.d_pos; p >= 0; p--) {  // ancestors of dof i = its body's chain up to the dof itself
      const int j = BYTE_OF(K.d_chain, p);
      double v = dot6(S(cdof) + 6 * j, buf);
      if (j == i) S(M)[MIDX(i, i)] = v + K.d_arm;
      else { S(M)[MIDX(i, j)] = v; S(M)[MIDX(j, i)] = v; }
    }
  }
  SYNC();
}

// ---- collision ---------------------------------------------------------------------------------------------
// "centre" index of a geom: its body id for agent geoms (one geom per moving body), nbody + w for world geom w.
// Positions / axes of all centres live in the xipos / gaxis arrays (world entries are written once per launch).
// The static collision tables (centre types / bodies / sizes, body invweights, world-geom frames and extents, dof chains)
// stay in device memory: a few hundred bytes that every wave of the CU reads (L1-resident).  SUMO_STAT_LDS=1 keeps them in
// LDS instead (2.2 KB per env for the Ant scene, which costs the seventh wave per CU).
#if SUMO_STAT_LDS
#define STAT_I(k) (c.si[c.L.stat_i + (k)])
#define STAT_D(k) (c.sm + c.L.stat_d + (k))
#else
#define STAT_I(k) (pt_global(c.P->aux.ai)[c.P->aux.o_stat_i + (k)])
#define STAT_D(k) (pt_global(c.P->aux.af) + c.P->aux.o_stat_d + (k))
#endif
#define CTYPE(ci) STAT_I(ci)
#define CBODY(ci) STAT_I(c.P->aux.nc + (ci))
#define CSIZE(ci) STAT_D(2 * (ci))
#define CINVW(ci) (STAT_D(2 * c.P->aux.nc + (ci))[0])
#define WBOX(w) STAT_D(3 * c.P->aux.nc + 12 * (w))
#define WLIM(w) STAT_D(3 * c.P->aux.nc + 12 * c.P->aux.nworld + 6 * (w))
#define CHAINW(b) (&STAT_I(2 * c.P->aux.nc + 2 * (b)))
#define CHLEN_AGENT(b) STAT_I(2 * c.P->aux.nc + 2 * c.P->mdl.nbody + (b))

__device__ __forceinline__ void make_frame(double* f) {
  if (f[3] * f[3] + f[4] * f[4] + f[5] * f[5] < 0.25) {
    f[3] = f[4] = f[5] = 0;
    if (f[1] < 0.5 && f[1] > -0.5) f[4] = 1; else f[5] = 1;
  }
  double dd = dot3(f, f + 3);
  f[3] -= f[0] * dd; f[4] -= f[1] * dd; f[5] -= f[2] * dd;
  normalize3(f + 3);
  cross3(f + 6, f, f + 3);
}

template <class C>
__device__ __forceinline__ void collision(C& c) {
  const int lane = c.lane, nb = c.P->mdl.nbody;
  // survivors of the broad phase (pair order preserved): pair ids and packed centre records (c1 | c2 << 8).  The queue
  // borrows the constraint-row arrays (jar / aref), which are dead until make_constraint.
  int* plist = (int*)S(jar);
  int* prlist = (int*)S(aref);
  int ncon = 0, dropped = 0;
  const auto& ax = aux_view(c);   // static-Layout variants: round counts are literals, the round loop unrolls completely
  const int WR = ax.wrounds, AR = ax.arounds, nwp = ax.nwp, maxcand = c.L.maxcand;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  // The pair table lists the pairs with a static world geom first (WR rounds of 64, padded), then the pairs between
  // moving geoms (AR rounds), contiguously.  The test is a chain of dependent loads (pair record -> centres in LDS / the
  // world geom's extent), so the rounds of both kinds are taken as ONE sequence, eight at a time, every record and bound of
  // a batch requested before the first test: Ant's 8 rounds are one batch (were three: 4-round batches, world and moving
  // pairs in separate loops).  A candidate with queue position in [base, base + maxcand) is stored, and the (rare)
  // overflow is handled by running the tests again for the next window.
  int base = 0, total = 0;
  do {
    int run = 0;
    const int PT_GAS* prp = pt_global(launder_ptr(c.prp));
    const float PT_GAS* pbp = pt_global(launder_ptr(c.pbp));
    constexpr int RB = 8;
    for (int r0 = 0; r0 < WR + AR; r0 += RB) {
      int rec[RB], pass[RB];
      float bnd[RB];
#pragma unroll
      for (int q = 0; q < RB; q++) {
        const int r = r0 + q;
        rec[q] = 0; bnd[q] = 0.f;
        if (r < WR + AR) { rec[q] = prp[WAVE * r]; bnd[q] = pbp[WAVE * r]; }
      }
#pragma unroll
      for (int q = 0; q < RB; q++) {
        const int r = r0 + q;
        pass[q] = 0;
        const double bound = (double)bnd[q];
        if (r < WR) {
          // world pair: distance from the moving geom's centre to the static geom's extent (box / segment / half space)
          const int ca = rec[q] & 0xFF, cw = (rec[q] >> 8) & 0xFF, w = cw >= nb ? cw - nb : 0;
          const double* pa = S(xipos) + 3 * ca;
          const double* pw = S(xipos) + 3 * cw;
          const double* bm = WBOX(w);
          const double* wl = WLIM(w);
          const double t[3] = {pa[0] - pw[0], pa[1] - pw[1], pa[2] - pw[2]};
          double ctr[3], d2 = 0;
          mulmatTvec3(ctr, bm, t);
#pragma unroll
          for (int k = 0; k < 3; k++) { double e = fmax(fmax(ctr[k] - wl[k], wl[3 + k] - ctr[k]), 0.0); d2 += e * e; }
          pass[q] = ((rec[q] >> 17) & 1) && !(d2 > bound * bound);
        } else if (r < WR + AR) {
          // pair of moving geoms: bounding spheres
          const double* p1 = S(xipos) + 3 * (rec[q] & 0xFF);
          const double* p2 = S(xipos) + 3 * ((rec[q] >> 8) & 0xFF);
          const double t[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
          pass[q] = ((rec[q] >> 17) & 1) && !(dot3(t, t) > bound * bound);
        }
      }
#pragma unroll
      for (int q = 0; q < RB; q++) {
        const int r = r0 + q;
        if (r < WR + AR) {
          const unsigned long long bal = __ballot(pass[q]);
          const int pos = run + __popcll(bal & lt_mask) - base;
          if (pass[q] && pos >= 0 && pos < maxcand) {
            const int ca = rec[q] & 0xFF, cw = (rec[q] >> 8) & 0xFF;
            if (r < WR) {
              plist[pos] = lane + WAVE * r;
              prlist[pos] = (rec[q] & (1 << 16)) ? (cw | (ca << 8)) : (ca | (cw << 8));   // bit 16: the world geom is geom1
            } else {
              plist[pos] = nwp + lane + WAVE * (r - WR);
              prlist[pos] = rec[q] & 0xFFFF;
            }
          }
          run += __popcll(bal);
        }
      }
    }
    total = run;
    const int ncand = total - base < maxcand ? total - base : maxcand;
    SYNC();
    PROF(4);
    for (int k0 = 0; k0 < ncand; k0 += WAVE) {
      int k = k0 + lane;
      Con1 cs[3];
      cs[0].ok = cs[1].ok = cs[2].ok = 0;
      int p = 0, b1 = 0, b2 = 0;
      double margin = 0;
      if (k < ncand) {
        p = plist[k];
        const int rc = prlist[k];
        const int c1 = rc & 0xFF, c2 = (rc >> 8) & 0xFF;
        const int t1 = CTYPE(c1), t2 = CTYPE(c2);  // cylinders already mapped to capsules (border rods)
        b1 = CBODY(c1); b2 = CBODY(c2);
        margin = c.P->mdl.fbase[c.P->mdl.o_pair_margin + p];
        const double* s1 = CSIZE(c1);
        const double* s2 = CSIZE(c2);
        const double* p1 = S(xipos) + 3 * c1;
        const double* p2 = S(xipos) + 3 * c2;
        const double* g1 = S(gaxis) + 3 * c1;
        const double* g2 = S(gaxis) + 3 * c2;
        double a1[3], a2[3];
        if (t1 == SUMO_GEOM_PLANE) {
          if (t2 == SUMO_GEOM_SPHERE) plane_sphere(cs[0], margin, p1, g1, p2, s2[0]);
          else if (t2 == SUMO_GEOM_CAPSULE) {
            double e[3];
            for (int q = 0; q < 3; q++) e[q] = p2[q] + g2[q] * s2[1];
            plane_sphere(cs[0], margin, p1, g1, e, s2[0]);
            for (int q = 0; q < 3; q++) e[q] = p2[q] - g2[q] * s2[1];
            plane_sphere(cs[1], margin, p1, g1, e, s2[0]);
          }
        } else if (t1 == SUMO_GEOM_SPHERE && t2 == SUMO_GEOM_SPHERE) {
          sphere_sphere(cs[0], margin, p1, s1[0], p2, s2[0]);
        } else if (t1 == SUMO_GEOM_SPHERE && t2 == SUMO_GEOM_CAPSULE) {
          double v[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
          double x = dot3(g2, v);
          if (x > s2[1]) x = s2[1];
          if (x < -s2[1]) x = -s2[1];
          double e[3] = {p2[0] + g2[0] * x, p2[1] + g2[1] * x, p2[2] + g2[2] * x};
          sphere_sphere(cs[0], margin, p1, s1[0], e, s2[0]);
        } else if (t1 == SUMO_GEOM_CAPSULE && t2 == SUMO_GEOM_CAPSULE) {
          for (int q = 0; q < 3; q++) { a1[q] = g1[q] * s1[1]; a2[q] = g2[q] * s2[1]; }
          double dif[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
          double ma = dot3(a1, a1), mb = -dot3(a1, a2), mc = dot3(a2, a2), u = -dot3(a1, dif), v = dot3(a2, dif);
          double det = ma * mc - mb * mb, v1[3], v2[3];
          if (fabs(det) >= MINVAL) {
            const double idet = fast_rcp(det), imc = fast_rcp(mc), ima = fast_rcp(ma);
            double x1 = (mc * u - mb * v) * idet, x2 = (ma * v - mb * u) * idet;
            if (x1 > 1) { x1 = 1; x2 = (v - mb) * imc; }
            else if (x1 < -1) { x1 = -1; x2 = (v + mb) * imc; }
            if (x2 > 1) { x2 = 1; x1 = (u - mb) * ima; if (x1 > 1) x1 = 1; else if (x1 < -1) x1 = -1; }
            else if (x2 < -1) { x2 = -1; x1 = (u + mb) * ima; if (x1 > 1) x1 = 1; else if (x1 < -1) x1 = -1; }
            for (int q = 0; q < 3; q++) { v1[q] = p1[q] + a1[q] * x1; v2[q] = p2[q] + a2[q] * x2; }
            sphere_sphere(cs[0], margin, v1, s1[0], v2, s2[0]);
          } else {
            for (int si = 0; si < 2; si++) {
              double sg = si == 0 ? 1.0 : -1.0;
              double x2 = (v - sg * mb) / mc;
              if (x2 > 1) x2 = 1; else if (x2 < -1) x2 = -1;
              for (int q = 0; q < 3; q++) { v1[q] = p1[q] + sg * a1[q]; v2[q] = p2[q] + a2[q] * x2; }
              if (si == 0) sphere_sphere(cs[0], margin, v1, s1[0], v2, s2[0]);
              else sphere_sphere(cs[1], margin, v1, s1[0], v2, s2[0]);
            }
          }
        } else if (t2 == SUMO_GEOM_BOX) {
          const double* bm = WBOX(c2 - nb);
          const double* bs = bm + 9;
          if (t1 == SUMO_GEOM_SPHERE) sphere_box(cs[0], margin, p1, s1[0], p2, bm, bs);
          else if (t1 == SUMO_GEOM_CAPSULE) {
            double axw[3] = {g1[0] * s1[1], g1[1] * s1[1], g1[2] * s1[1]}, e[3];
            for (int q = 0; q < 3; q++) e[q] = p1[q] + axw[q];
            sphere_box(cs[0], margin, e, s1[0], p2, bm, bs);
            for (int q = 0; q < 3; q++) e[q] = p1[q] - axw[q];
            sphere_box(cs[1], margin, e, s1[0], p2, bm, bs);
            double t[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]}, cc[3], a[3];
            mulmatTvec3(cc, bm, t);
            mulmatTvec3(a, bm, axw);
            double glo = seg_box_dgrad(cc, a, bs, -1.0), ghi = seg_box_dgrad(cc, a, bs, 1.0);
            if (glo < 0 && ghi > 0) {
              // the derivative is piecewise linear and non-decreasing in t: bracket the root between consecutive
              // breakpoints (where a coordinate crosses a box face), then interpolate exactly
              double lo = -1, hi = 1;
#pragma unroll
              for (int k = 0; k < 3; k++) {
                const double ra = fast_rcp(a[k]);
#pragma unroll
                for (int sg = 0; sg < 2; sg++) {
                  const double tb = ((sg ? -bs[k] : bs[k]) - cc[k]) * ra;
                  if (tb > lo && tb < hi) {
                    const double gb = seg_box_dgrad(cc, a, bs, tb, k);
                    if (gb > 0) { hi = tb; ghi = gb; } else { lo = tb; glo = gb; }
                  }
                }
              }
              double ts = lo - glo * (hi - lo) * fast_rcp(ghi - glo);
              for (int q = 0; q < 3; q++) e[q] = p1[q] + ts * axw[q];
              sphere_box(cs[2], margin, e, s1[0], p2, bm, bs);
            }
          }
        }
      }
      int act[3], n = 0;
#pragma unroll
      for (int q = 0; q < 3; q++) { act[q] = cs[q].ok && (cs[q].dist < margin); n += act[q]; }
      int ctot, cbase = wave_excl_scan(n, lane, &ctot);
      int slot = ncon + cbase;
#pragma unroll
      for (int q = 0; q < 3; q++) {
        if (act[q]) {
          if (slot < c.L.maxcon) {
            double* cd = S(cond) + 14 * slot;
            double fr[9] = {cs[q].nrm[0], cs[q].nrm[1], cs[q].nrm[2], 0, 0, 0, 0, 0, 0};
            make_frame(fr);
            cd[0] = cs[q].dist; cd[1] = cs[q].pos[0]; cd[2] = cs[q].pos[1]; cd[3] = cs[q].pos[2];
            for (int w = 0; w < 9; w++) cd[4 + w] = fr[w];
            cd[13] = 0;
            int* cb = c.si + c.L.con_b + 4 * slot;
            cb[0] = b1; cb[1] = b2; cb[2] = p; cb[3] = 0;
          }
          slot++;
        }
      }
      ncon += ctot;
    }
    SYNC();
    PROF(5);
    base += maxcand;
  } while (base < total);
  if (ncon > c.L.maxcon) { dropped = ncon - c.L.maxcon; ncon = c.L.maxcon; }
  c.ncon = ncon;
  c.ndropped = dropped;
  SYNC();
#ifndef SUMO_NO_FIDELITY
  // contact-generation fidelity accounting (Ctx::st_cb3), out of line (the narrow-phase loop above stays as it was) and SAMPLED: the
  // forward evaluation that opens an env step, 1 in frame_skip x 4 RK stages = 20 (every forward: +0.9 % on the bench; sampled: nil)
  if ((c.st_forward - 1) % 20 == 0) {
    const auto& mdl = model_view(c);
    const int r = fidelity_count(S(cond), c.si + c.L.con_b, ncon, lane, MI(pair_geom2), MI(geom_type), MF(geom_pos), MF(geom_quat), MF(geom_size));
    c.st_cb3 += r & 0xFFFF;
    c.st_rodcap += r >> 16;
  }
#endif
}

// ---- constraint rows -----------------------------------------------------------------------------------------
__device__ __noinline__ double impedance_general_pow(double xx, double mid, double power) {  // rare: power not in {1, 2}
  if (xx <= mid) return pow(xx, power) / pow(mid, power - 1);
  return 1 - pow(1 - xx, power) / pow(1 - mid, power - 1);
}
__device__ __forceinline__ double impedance(const double* solimp, double x) {
  double dmin = solimp[0], dmax = solimp[1], width = solimp[2], mid = solimp[3], power = solimp[4];
  dmin = fmin(fmax(dmin, 0.0001), 0.9999);
  dmax = fmin(fmax(dmax, 0.0001), 0.9999);
  if (width < MINVAL) width = MINVAL;
  mid = fmin(fmax(mid, 0.0001), 0.9999);
  if (power < 1) power = 1;
  double xx = fabs(x) * fast_rcp(width), y;
  if (xx >= 1) return dmax;
  if (xx <= 0) return dmin;
  if (power == 1) y = xx;
  else if (power == 2) y = xx <= mid ? xx * xx * fast_rcp(mid) : 1 - (1 - xx) * (1 - xx) * fast_rcp(1 - mid);  // MuJoCo default solimp
  else y = impedance_general_pow(xx, mid, power);
  return dmin + y * (dmax - dmin);
}
// returns R; writes B and K*imp*(pos-margin)
__device__ __forceinline__ double row_params(double timestep, const double* solref, const double* solimp, double pos, double margin,
                                             double diag, double* B, double* kterm) {
  double tc = solref[0], dr = solref[1], dmax = fmin(fmax(solimp[1], 0.0001), 0.9999);
  if (tc < 2 * timestep) tc = 2 * timestep;
  double imp = impedance(solimp, pos - margin);
  double kk = dmax * dmax * tc * tc * dr * dr, bb = dmax * tc;
  double K = fast_rcp(kk < MINVAL ? MINVAL : kk);
  *B = 2.0 * fast_rcp(bb < MINVAL ? MINVAL : bb);
  *kterm = K * imp * (pos - margin);
  double R = (1 - imp) * diag * fast_rcp(imp);
  return R < MINVAL ? MINVAL : R;
}

template <class C>
__device__ __forceinline__ void make_constraint(C& c) {
  const auto& mdl = model_view(c);
  KCONSTS();
  const int lane = c.lane, nv = mdl.nv;
  // ---- Jacobian pool allocation (contact order): one 3x8 half per moving body of the contact
  int ncon = c.ncon;
  {
    int nh = 0;
    int* cb = c.si + c.L.con_b + 4 * (lane < ncon ? lane : 0);
    if (lane < ncon) nh = (cb[0] != 0 && cb[1] != 0) ? 2 : 1;
    int tot, pre = wave_excl_scan(nh, lane, &tot);
    unsigned long long nofit = __ballot(lane < ncon && pre + nh > c.L.jbcap);
    if (nofit) { int nfit = __builtin_ctzll(nofit); c.ndropped += ncon - nfit; ncon = nfit; c.ncon = nfit; }
    if (lane < ncon) cb[3] = (24 * pre) | ((nh == 2) << 20);
    SYNC();
  }
  const double timestep = MF(opt)[SUMO_OPT_TIMESTEP];
  OPAQUE_F64(sr0_, 0.02); OPAQUE_F64(si0_, 0.9); OPAQUE_F64(si1_, 0.95); OPAQUE_F64(si2_, 0.001);   // MuJoCo's default solref / solimp
  const double def_solref[2] = {sr0_, 1.0};
  const double def_solimp[5] = {si0_, si1_, si2_, 0.5, 2.0};
  // joint limits; lane == joint id.  A hinge owns two fixed slots indexed by its dof (lower side, upper side): D = 1/R and
  // aref, with D = 0 when the side is not active (every term of the solver carries D, so absent rows cost nothing).
  // The Jacobian of a limit row is +-e_dof: the dof's own lane evaluates its rows without touching LDS row arrays.
  int act_lo = 0, act_hi = 0;
  if (lane < nv) ((unsigned long long*)S(cmask))[lane] = 0ull;
  if (lane < mdl.njnt && role_jt_hinge(c)) {
    const int dof = role_jt_dadr(c), limited = role_jt_limited(c);
    const double jm = K.jt_margin, value = S(qpos)[role_jt_qadr(c)], vel = S(qvel)[dof];
    const double dlo = value - K.jt_lo, dhi = K.jt_hi - value;
    act_lo = limited && dlo < jm; act_hi = limited && dhi < jm;
    double D0 = 0, A0 = 0, D1 = 0, A1 = 0;
    // one evaluation per lane, of the side that is active (a wave with hinges at their lower and others at their upper limit
    // -- the usual case -- runs the body once, not once per side)
    if (act_lo || act_hi) {
      double B, kt, R = row_params(timestep, def_solref, def_solimp, act_lo ? dlo : dhi, jm, K.jt_invw, &B, &kt);
      const double Dr = fast_rcp(R), Alo = -B * vel - kt, Ahi = B * vel - kt;     // upper side: row = -e_dof, efc_vel = -qvel
      D0 = act_lo ? Dr : 0.0; A0 = act_lo ? Alo : 0.0;
      D1 = act_lo ? 0.0 : Dr; A1 = act_lo ? 0.0 : Ahi;
    }
    // both sides of one hinge active: only where its range is narrower than twice the margin.  The test is uniform over the
    // lanes here, so a wave without such a hinge skips the second evaluation.
    if (__ballot(act_lo && act_hi) != 0ull) {
      if (act_lo && act_hi) {
        double B, kt, R = row_params(timestep, def_solref, def_solimp, dhi, jm, K.jt_invw, &B, &kt);
        D1 = fast_rcp(R); A1 = B * vel - kt;
      }
    }
    const int hid = role_jt_hid(c), nh = c.L.nhinge;
    S(limD)[hid] = D0; S(limD)[nh + hid] = D1; S(limA)[hid] = A0; S(limA)[nh + hid] = A1;
  }
  const int nlim = __popcll(__ballot(act_lo)) + __popcll(__ballot(act_hi));
  SYNC();
  c.nlim = nlim;
  c.nefc = nlim + 4 * ncon;
  {
    int two = 0, cross = 0;
    const int b1 = MI(agent_bodyadr)[1];
    for (int ci = lane; ci < ncon; ci += WAVE) {
      const int* cb = c.si + c.L.con_b + 4 * ci;
      if (cb[0] != 0 && cb[1] != 0) { two = 1; if ((cb[0] >= b1) != (cb[1] >= b1)) cross = 1; }
    }
    c.htree = c.L.tree_ok && !c.L.force_dense && __ballot(two) == 0ull;
#ifdef SUMO_DBG_DUMP
    // development builds (-DSUMO_DBG_DUMP, the build tools/dump_diff.py runs): on the tree path every contact took
    // one 3 x 8 block of the pool, so the offset of contact ci is 24 ci -- what tree_rows, contact_Jx<8> and the tree-path gradient
    // rely on.  `ncon` is the count after the pool's capacity cut (at most maxcon, which is below 64: one contact per lane, word 4 * lane + 3).
    assert(!(c.htree && lane < ncon && (c.si + c.L.con_b)[4 * lane + 3] != 24 * lane));
#endif
    c.hcross = __ballot(cross) != 0ull;
  }
  // contact row parameters (same for the 4 pyramid edges of a contact)
  for (int ci = lane; ci < ncon; ci += WAVE) {
    const double* cd = S(cond) + 14 * ci;
    const int* cb = c.si + c.L.con_b + 4 * ci;
    int p = cb[2];
    double mu = MF(pair_friction)[3 * p];
    double pm = MF(pair_margin)[p], pg = MF(pair_gap)[p];
    double sr[2] = {MF(pair_solref)[2 * p], MF(pair_solref)[2 * p + 1]};
    double si_[5];
    for (int q = 0; q < 5; q++) si_[q] = MF(pair_solimp)[5 * p + q];
    double tran = CINVW(cb[0]) + CINVW(cb[1]);   // body ids double as centre ids (world body 0 -> 0)
    double diag = tran + mu * mu * tran, B, kt;
    double R = row_params(timestep, sr, si_, cd[0], pm - pg, diag, &B, &kt);
    double Rpy = 2 * mu * mu * R;
    if (Rpy < MINVAL) Rpy = MINVAL;
    S(cpar)[ci] = mu;
    S(D)[ci] = fast_rcp(Rpy);   // one D per contact (its four pyramid rows share it)
    for (int k = 0; k < 4; k++) { int r = 4 * ci + k; S(aref)[r] = B; S(jar)[r] = kt; }
  }
  PROF(6);
  // compact contact Jacobians: 3 base rows (normal, t1, t2) x ns slots.  Two moving bodies: ns = 16 (chain of body1,
  // sign -, then chain of body2, sign +); one moving body (contact with the world): ns = 8, that body's chain only.
  for (int idx = lane; idx < ncon * 16; idx += WAVE) {
    int ci = idx >> 4, s = idx & 15;
    const int* cb = c.si + c.L.con_b + 4 * ci;
    const int two = cb[3] >> 20, jb = cb[3] & 0xFFFFF, ns = two ? 16 : 8;
    int side, pos = s & 7;
    bool slot_ok = true;
    if (two) side = s >> 3;
    else { side = cb[0] != 0 ? 0 : 1; slot_ok = s < 8; }
    int body = side ? cb[1] : cb[0], other = side ? cb[0] : cb[1];
    int dof = -1, ag = 0;
    double j0 = 0, j1 = 0, j2 = 0;
    if (slot_ok && body != 0) {
      int la = CHLEN_AGENT(body);
      ag = la >> 8;
      if (pos < (la & 0xFF)) {
        const int* cw = CHAINW(body);
        dof = ((unsigned)cw[pos >> 2] >> (8 * (pos & 3))) & 0xFF;
        // a dof shared by both bodies' root paths sits at the same chain position: its contributions cancel
        if (other != 0 && pos < (CHLEN_AGENT(other) & 0xFF)) {
          const int* ow = CHAINW(other);
          if ((int)(((unsigned)ow[pos >> 2] >> (8 * (pos & 3))) & 0xFF) == dof) dof = -1;
        }
      }
    }
    if (dof >= 0) {
      const double* cd = S(cond) + 14 * ci;
      const double* cdf = S(cdof) + 6 * dof;
      double off[3] = {cd[1] - S(com)[3 * ag], cd[2] - S(com)[3 * ag + 1], cd[3] - S(com)[3 * ag + 2]}, t[3];
      cross3(t, cdf, off);
      t[0] += cdf[3]; t[1] += cdf[4]; t[2] += cdf[5];
      double sg = side ? 1.0 : -1.0;
      j0 = sg * dot3(cd + 4, t); j1 = sg * dot3(cd + 7, t); j2 = sg * dot3(cd + 10, t);
      atomicOr((unsigned long long*)S(cmask) + dof, 1ull << ci);
    }
    ((signed char*)c.sb)[c.L.b_dofidx + idx] = (signed char)dof;
    if (slot_ok) {
      double* Jb = S(Jb) + jb;
      Jb[s] = j0; Jb[ns + s] = j1; Jb[2 * ns + s] = j2;
    }
  }
  SYNC();
  PROF(7);
}

// Jacobian slot of dof `d` in contact `ci`: slots are positions in the dof chain of the contact's body (second body: + 8);
// `p` is the dof's position in its own body's chain, which is also its position in the chain of any body below it
#define SLOT_OF(ci, d, p) ((((const signed char*)c.sb)[c.L.b_dofidx + 16 * (ci) + (p)] == (signed char)(d)) ? (p) : (p) + 8)
// cp[3*c + a] = sum_s Jb[c][a][s] * x[dof(c,s)].  Branch-free and fully unrolled so all 16 slot loads are in flight at
// once: Jb is exactly 0 in unused slots, so those may read any x.
// NS == 8 (the tree path, c.htree): every contact has one moving body, so its block is 3 x 8 at 24 * ci (make_constraint) and slots
// 8 .. 15 do not exist.  The general form gives those slots jv = 0: each adds 0.0 * x to an accumulator that is never -0 (it starts at
// +0, and an exact zero sum rounds to +0), so for finite x leaving them out changes no bit.  A non-finite x belongs to an env that the
// divergence guard replaces at the end of the step.
template <int NS = 16, class C>
__device__ __forceinline__ void contact_Jx(C& c, const double* x) {
  for (int idx = c.lane; idx < 3 * c.ncon; idx += WAVE) {
    int ci = idx / 3, a = idx - 3 * ci;
    const signed char* di = (const signed char*)c.sb + c.L.b_dofidx + 16 * ci;
    double xv[NS], jv[NS];
    if constexpr (NS == 8) {
      const double* Jb = S(Jb) + 24 * ci + 8 * a;
#pragma unroll
      for (int s = 0; s < 8; s++) { int d = di[s]; xv[s] = x[d < 0 ? 0 : d]; jv[s] = Jb[s]; }
    } else {
      const int info = (c.si + c.L.con_b)[4 * ci + 3], ns = (info >> 20) ? 16 : 8;
      const double* Jb = S(Jb) + (info & 0xFFFFF) + ns * a;
#pragma unroll
      for (int s = 0; s < 16; s++) { int d = di[s]; xv[s] = x[d < 0 ? 0 : d]; double jq = Jb[s]; jv[s] = s < ns ? jq : 0.0; }
    }
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
    for (int s = 0; s < NS; s += 4) { a0 += jv[s] * xv[s]; a1 += jv[s + 1] * xv[s + 1]; a2 += jv[s + 2] * xv[s + 2]; a3 += jv[s + 3] * xv[s + 3]; }
    S(cp)[idx] = (a0 + a1) + (a2 + a3);
  }
  SYNC();
}
// The same products for three vectors in one pass over the slots (the solver set-up: warm start, qacc_smooth, qvel): a
// slot's Jb words and dof indices are loaded once, the vectors are taken in turn against that one set of jv[16], and each
// keeps contact_Jx's a0..a3 grouping, so every cp word carries the bits the single pass gives.  cp0..cp2 are offsets in c.sm.
template <int NS = 16, class C>   // NS == 8: the tree path, as in contact_Jx
__device__ __forceinline__ void contact_Jx3(C& c, const double* x0, const double* x1, const double* x2, int cp0, int cp1, int cp2) {
  for (int idx = c.lane; idx < 3 * c.ncon; idx += WAVE) {
    int ci = idx / 3, a = idx - 3 * ci;
    const signed char* di = (const signed char*)c.sb + c.L.b_dofidx + 16 * ci;
    double jv[NS];
    int dv[NS];
    if constexpr (NS == 8) {
      const double* Jb = S(Jb) + 24 * ci + 8 * a;
#pragma unroll
      for (int s = 0; s < 8; s++) { int d = di[s]; dv[s] = d < 0 ? 0 : d; jv[s] = Jb[s]; }
    } else {
      const int info = (c.si + c.L.con_b)[4 * ci + 3], ns = (info >> 20) ? 16 : 8;
      const double* Jb = S(Jb) + (info & 0xFFFFF) + ns * a;
#pragma unroll
      for (int s = 0; s < 16; s++) { int d = di[s]; dv[s] = d < 0 ? 0 : d; double jq = Jb[s]; jv[s] = s < ns ? jq : 0.0; }
    }
#pragma unroll
    for (int v = 0; v < 3; v++) {
      const double* x = v == 0 ? x0 : (v == 1 ? x1 : x2);
      double xv[NS];
#pragma unroll
      for (int s = 0; s < NS; s++) xv[s] = x[dv[s]];
      double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
      for (int s = 0; s < NS; s += 4) { a0 += jv[s] * xv[s]; a1 += jv[s + 1] * xv[s + 1]; a2 += jv[s + 2] * xv[s + 2]; a3 += jv[s + 3] * xv[s + 3]; }
      c.sm[(v == 0 ? cp0 : (v == 1 ? cp1 : cp2)) + idx] = (a0 + a1) + (a2 + a3);
    }
  }
  SYNC();
}
// value of contact row r (= 4 * contact + pyramid edge) of J*x given its cp words at offset `cpo` of c.sm
template <class C>
__device__ __forceinline__ double row_Jx_at(const C& c, int cpo, int r) {
  const int ci = r >> 2, k = r & 3;
  double mu = c.sm[c.L.cpar + ci];
  const double* cp = c.sm + cpo + 3 * ci;
  return cp[0] + ((k & 1) ? -mu : mu) * cp[1 + (k >> 1)];
}
// ... given cp (after contact_Jx)
template <class C>
__device__ __forceinline__ double row_Jx(const C& c, int r) { return row_Jx_at(c, c.L.cp, r); }
// this lane's two joint-limit slots (lower, upper): D (0 = absent) and aref
struct LimRows { double D0, D1, A0, A1; };
template <class C>
__device__ __forceinline__ LimRows lim_rows(const C& c) {
  const int nh = c.L.nhinge, hid = role_d_hid(c), h = hid < 0 ? 0 : hid;
  LimRows q;
  q.D0 = c.sm[c.L.limD + h]; q.D1 = c.sm[c.L.limD + nh + h]; q.A0 = c.sm[c.L.limA + h]; q.A1 = c.sm[c.L.limA + nh + h];
  if (hid < 0) q.D0 = q.D1 = 0.0;     // free-joint dofs and lanes past nv carry no limit
  return q;
}

// y_i = sum_k M[i][k] x[k]   (x in LDS); M is block diagonal, so only the lane's own tree contributes
template <class C>
__device__ __forceinline__ double dense_Mx(const C& c, const double* x) {
  constexpr int NV = C::NV;
  double acc = 0;
  if (c.L.d1 * 2 == NV) {  // two equal trees: fixed trip count, all loads issued up front
    const int li = c.lane < NV ? c.lane : 0;
    const int k0 = li >= NV / 2 ? NV / 2 : 0;
    const double* row = c.sm + c.L.M + li * c.L.mld;
    double a0 = 0, a1 = 0;
#pragma unroll
    for (int k = 0; k < NV / 2; k += 2) { a0 += row[k] * x[k0 + k]; a1 += row[k + 1] * x[k0 + k + 1]; }
    acc = c.lane < NV ? a0 + a1 : 0.0;
  } else if (c.lane < c.P->mdl.nv) {
    const int d1 = c.L.d1, nv = c.P->mdl.nv;
    const int k0 = c.lane >= d1 ? d1 : 0, k1 = c.lane >= d1 ? nv : d1;
    const double* row = c.sm + c.L.M + c.lane * c.L.mld;
    for (int k = k0; k < k1; k++) acc += row[k - k0] * x[k];
  }
  return acc;
}

// Solve A x = b for a symmetric positive definite A held in LDS (packed lower triangle): lane i loads row i
// into registers, the wave runs a right-looking LDL^T entirely with v_readlane broadcasts (no LDS traffic, no barriers;
// fully unrolled so every register index is static), forward-substitutes, transposes L through LDS once (`T`, packed)
// and back-substitutes.  Lane i holds b_i on entry and returns x_i.  *fail is wave-uniform.
// This is the general path (a contact between two moving bodies fills H outside the tree pattern).
template <class C>
__device__ __forceinline__ double ldl_solve_rows(C& c, const double* A, double* T, double b, int* fail) {
  constexpr int NV = C::NV;
  const int lane = c.lane;
  const int li = lane < NV ? lane : NV - 1;
  double a[NV];
#pragma unroll
  for (int k = 0; k < NV; k++) a[k] = A[HP(li, (k <= li ? k : li))];
  double dinv = 0;
  int bad = 0;
#pragma unroll
  for (int j = 0; j < NV; j++) {
    double ajj = readlane_f64(a[j], j);
    if (ajj < MINVAL) bad = 1;
    double r = fast_rcp(ajj);
    double lij = a[j] * r;
#pragma unroll
    for (int k = j + 1; k < NV; k++) a[k] -= lij * readlane_f64(a[j], k);  // lanes < k only touch unused entries
    if (lane == j) dinv = r;
    a[j] = lij;
  }
  double y = b;
#pragma unroll
  for (int k = 0; k < NV - 1; k++) {
    double yk = readlane_f64(y, k);
    if (lane > k) y -= a[k] * yk;
  }
  y *= dinv;
  // write L back into the packed triangle (row `lane`), then every lane reads its COLUMN from there (back substitution)
  {
    const int rbase = HP(li, 0);
#pragma unroll
    for (int k = 0; k < NV - 1; k++)
      if (lane > k && lane < NV) T[rbase + k] = a[k];
  }
  SYNC();
  double t[NV];
#pragma unroll
  for (int k = 1; k < NV; k++) t[k] = T[HP(k, li)];   // L[k][lane]; entries with k <= lane are never used
#pragma unroll
  for (int k = NV - 1; k > 0; k--) {
    double xk = readlane_f64(y, k);
    if (lane < k) y -= t[k] * xk;
  }
  SYNC();
  *fail = bad;
  return y;
}

// ---- tree-sparse factorisation ----------------------------------------------------------------------------------
// Every agent of the nine scenes is a free body (6 dofs) carrying legs of two hinges (hip, ankle), with the dofs ordered
// root 0..5, then (hip, ankle) per leg (checked on the host, Layout::tree_ok).  The mass matrix -- and the Newton
// Hessian as long as every contact touches a single moving body -- is then nonzero only between a dof and its
// ancestors: lane i keeps row i as row[p] = A[i][ancestor at chain position p] (root dof m: p <= m; hip: 0..5 root,
// 6 diag; ankle: 0..5 root, 6 hip, 7 diag).  A x = b is solved by block elimination (MuJoCo's mj_factorM order, leaves
// first): the 2x2 leg blocks are inverted in their own lanes, the 6x6 Schur complement of each root is accumulated one
// needed word per lane and factorised redundantly by every lane of the agent.  No fill-in, five short phases.
#define DPP_SWAP_PAIR 0xB1  /* quad_perm [1,0,3,2]: exchange with the neighbouring lane (hip <-> ankle; hips sit on even lanes) */
__device__ __forceinline__ double pair_swap_f64(double v) {
  return dpp_mov_f64<DPP_SWAP_PAIR>(v);   // every lane has a source
}

// row <- tree row `lane` of M + diag_add on the diagonal (+ J^T W J of the contacts touching this dof)
template <class C>
__device__ __forceinline__ void tree_rows(C& c, double (&row)[8], double diag_add, bool with_contacts) {
  const int lane = c.lane, nv = c.P->mdl.nv, d1 = c.L.d1;
  const int li = lane < nv ? lane : 0;
  const int il = li >= d1 ? li - d1 : li;           // dof index inside the agent
  const int pos = il < 6 ? il : 6 + (il & 1);       // chain position of the dof itself
  const double* Mrow = S(M) + li * c.L.mld;
#pragma unroll
  for (int p = 0; p < 6; p++) row[p] = Mrow[p] + (p == il ? diag_add : 0.0);
  const double mh = Mrow[il < 6 ? 0 : il - (il & 1)], md = Mrow[il];   // column of the leg's hip, own diagonal
  row[6] = il < 6 ? 0.0 : ((il & 1) ? mh : md + diag_add);
  row[7] = (il >= 6 && (il & 1)) ? md + diag_add : 0.0;
  if (with_contacts && lane < nv) {
    for (unsigned long long mk = ((const unsigned long long*)S(cmask))[lane]; mk; mk &= mk - 1) {
      const int ci = __builtin_ctzll(mk);
      const double* Jb = S(Jb) + 24 * ci;   // one moving body per contact: 3 rows x 8 chain slots, the pool offset is 24 ci (make_constraint)
      const double* W = S(cW) + 5 * ci;
      const double a0 = Jb[pos], a1 = Jb[8 + pos], a2 = Jb[16 + pos];
      const double u0 = W[0] * a0 + W[1] * a1 + W[2] * a2, u1 = W[1] * a0 + W[3] * a1, u2 = W[2] * a0 + W[4] * a2;
#pragma unroll
      for (int p = 0; p < 8; p++) row[p] += u0 * Jb[p] + u1 * Jb[8 + p] + u2 * Jb[16 + p];   // slots past `pos` are unused entries
    }
  }
}

template <class C>
__device__ __forceinline__ double tree_factor_solve(C& c, const double (&row)[8], double b, int* fail) {
  const int lane = c.lane, nv = c.P->mdl.nv, d1 = c.L.d1;
  const bool act = lane < nv;
  const int B = lane >= d1 ? d1 : 0, il = lane - B;
  const bool isleg = act && il >= 6, iship = !(il & 1);
  double* ROW = S(H);           // [nv][8] rows (root rows are overwritten by the Schur complement: [0..5] S, [6] rhs)
  double* WW = S(H) + 8 * nv;   // [nv][6] leg dofs: row of A_ll^-1 A_lr
  double* Y = S(tmpv);          // [nv]    leg dofs: A_ll^-1 b_l
  int bad = 0;
  // ---- leg blocks: [[dh, o], [o, da]] (hip, ankle); each lane computes its own row of the inverse applied to (A_lr | b_l)
  double pr[8];
#pragma unroll
  for (int p = 0; p < 8; p++) pr[p] = pair_swap_f64(row[p]);
  const double pb = pair_swap_f64(b);
  const double d_own = iship ? row[6] : row[7], d_par = iship ? pr[7] : pr[6], off = iship ? pr[6] : row[6];
  const double det = d_own * d_par - off * off;
  if (isleg && (d_par < MINVAL || det < MINVAL * d_par)) bad = 1;   // pivots of the 2x2 LDL: d_par, det / d_par
  const double idet = fast_rcp(det);
  double w[6];
#pragma unroll
  for (int p = 0; p < 6; p++) w[p] = (d_par * row[p] - off * pr[p]) * idet;
  const double y = (d_par * b - off * pb) * idet;
  if (act) {
#pragma unroll
    for (int p = 0; p < 6; p++) ROW[8 * lane + p] = row[p];
    ROW[8 * lane + 6] = b;   // a root row's right-hand side, the start of its Schur word; nobody reads words 6 / 7 of a leg row
    if (isleg) {
#pragma unroll
      for (int p = 0; p < 6; p++) WW[6 * lane + p] = w[p];
      Y[lane] = y;
    }
  }
  SYNC();
  // ---- Schur complement of the root block: S = A_rr - A_rl A_ll^-1 A_lr, rhs' = b_r - A_rl A_ll^-1 b_l, one lane per word the
  // factorisation below reads: per agent the 21 words S[i][j], j <= i, and the 6 of the right-hand side (word 6 of row i) -- lanes
  // 0 .. 26 agent 0, 27 .. 53 agent 1.  Entry t of an agent: t = 7 r + q; r < 3 pairs row r (q <= r) with row 5 - r (7 words
  // together), r == 3 is the right-hand side of row q.  A word starts from what phase 1 stored there and takes its leg dofs in
  // ascending order, every product subtracted by one fma: the chain, the operands and the order of the row-per-lane form this
  // replaces, so the bits are the same.  Each word is read and written by its own lane only; leg rows, WW and Y are only read.
  {
    int e = lane;
    asm volatile("" : "+v"(e));   // opaque: the entry's integers are formed here, per call, not once per launch and kept in registers
    const int ag = e >= 27, t = e - 27 * ag, r = (t * 37) >> 8, q = t - 7 * r;   // (t * 37) >> 8 == t / 7 for t < 28
    const bool rhs = r == 3, lo = q <= r;
    const int i = rhs ? q : (lo ? r : 5 - r), j = rhs ? 6 : (lo ? q : q - r - 1);
    const int Be = ag ? d1 : 0, nld = (ag ? nv - d1 : d1) - 6, d0 = Be + 6;   // first leg dof of the entry's agent
    // leg dofs of the agent: at most MAXLD; unrolled over the bound with every load issued before the FMAs (a leg dof past the
    // agent's own re-reads the first one and is masked out of the sum)
    constexpr int MAXLD = C::NV == 28 ? 8 : (C::NV == 32 ? 12 : 16);
    if (e < 54) {
      double* own = ROW + 8 * (Be + i) + j;
      const double* pa = ROW + 8 * d0 + i;
      const double* sm = c.sm;
      const int wo = rhs ? c.L.tmpv + d0 : c.L.H + 8 * nv + 6 * d0 + j, ws = rhs ? 1 : 6;   // Y[d] or WW[6 d + j]
      double s = *own, am[MAXLD], wv[MAXLD];
#pragma unroll
      for (int k = 0; k < MAXLD; k++) {
        const int kk = k < nld ? k : 0;
        am[k] = pa[8 * kk];
        wv[k] = sm[wo + ws * kk];
      }
#pragma unroll
      for (int k = 0; k < MAXLD; k++) s = __builtin_fma(-(k < nld ? am[k] : 0.0), wv[k], s);
      *own = s;
    }
  }
  SYNC();
  // ---- 6x6 LDL^T + solve, redundantly in every lane of the agent
  double L[6][6], xr[6];
  {
    const double* Sg = ROW + 8 * B;
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
      for (int j = 0; j <= i; j++) L[i][j] = Sg[8 * i + j];
      xr[i] = Sg[8 * i + 6];
    }
    double rinv[6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
      if (act && L[j][j] < MINVAL) bad = 1;
      rinv[j] = fast_rcp(L[j][j]);
      double u[6];
#pragma unroll
      for (int i = j + 1; i < 6; i++) u[i] = L[i][j];
#pragma unroll
      for (int i = j + 1; i < 6; i++) {
        const double lij = u[i] * rinv[j];
#pragma unroll
        for (int k = j + 1; k <= i; k++) L[i][k] -= lij * u[k];
        L[i][j] = lij;
      }
    }
#pragma unroll
    for (int i = 1; i < 6; i++)
#pragma unroll
      for (int j = 0; j < i; j++) xr[i] -= L[i][j] * xr[j];
#pragma unroll
    for (int i = 0; i < 6; i++) xr[i] *= rinv[i];
#pragma unroll
    for (int i = 4; i >= 0; i--)
#pragma unroll
      for (int k = i + 1; k < 6; k++) xr[i] -= L[k][i] * xr[k];
  }
  // ---- back substitution into the legs: x_l = A_ll^-1 b_l - (A_ll^-1 A_lr) x_r
  double x = y;
#pragma unroll
  for (int p = 0; p < 6; p++) x -= w[p] * xr[p];
#pragma unroll
  for (int p = 0; p < 6; p++) x = il == p ? xr[p] : x;
  SYNC();
  *fail = __ballot(bad) != 0ull;
  return act ? x : 0.0;
}

// cost(x) = 1/2 (Ma - qfrc_smooth).(x - qacc_smooth) + sum_active 1/2 D jar^2   (jar of the contact rows in LDS; the
// limit rows of a dof are evaluated by its lane: jar = +-x - aref)
template <class C>
__device__ __forceinline__ double solver_cost_part(C& c, double Ma_i, double x_i) {   // this lane's share, before the wave sum
  const int lane = c.lane, nv = c.P->mdl.nv;
  double v = 0;
  if (lane < nv) v = 0.5 * (Ma_i - S(qsm)[lane]) * (x_i - S(asmo)[lane]);
  const LimRows q = lim_rows(c);
  const double j0 = x_i - q.A0, j1 = -x_i - q.A1;
  if (j0 < 0) v += 0.5 * q.D0 * j0 * j0;
  if (j1 < 0) v += 0.5 * q.D1 * j1 * j1;
  for (int r = lane; r < 4 * c.ncon; r += WAVE) { double j = S(jar)[r]; if (j < 0) v += 0.5 * S(D)[r >> 2] * j * j; }
  return v;
}
template <class C>
__device__ __forceinline__ double solver_cost(C& c, double Ma_i, double x_i) { return wave_sum(solver_cost_part(c, Ma_i, x_i)); }

// TREE: every contact touches one moving body (c.htree) -- two instantiations so that the register-hungry general
// factorisation does not share a loop (and its spills) with the common tree-sparse one
template <bool TREE, class C>
__device__ __forceinline__ void newton_solve(C& c) {
  const auto& mdl = model_view(c);
  const auto& aux = aux_view(c);
  const int lane = c.lane, nv = mdl.nv, nefc = c.nefc, ncon = c.ncon, nrow = 4 * c.ncon;
  const double tol = MF(opt)[SUMO_OPT_TOLERANCE];
  const int maxiter = (int)MF(opt)[SUMO_OPT_ITERATIONS];
  const double scale = 1.0 / (MF(opt)[SUMO_OPT_MEANINERTIA] * (nv > 1 ? nv : 1));
  double* x = S(x);
  if (nefc == 0) {
    if (lane < nv) x[lane] = S(asmo)[lane];
    SYNC();
    return;
  }
  constexpr int RPL = C::NV <= 36 ? 2 : 3;   // contact rows per lane: 4 * maxcon <= 64 * RPL (build_layout)
  // ---- warm start: better of qacc_warmstart (or, in warm_mode 1, the previous RK stage's qacc still held in x) and
  // qacc_smooth
  if (!c.use_prev && lane < nv) x[lane] = S(warm)[lane];
  SYNC();
  double Ma = dense_Mx(c, x);
  // one pass over the contact Jacobians for J x, J qacc_smooth and J qvel (efc_vel).  The two extra cp buffers: cW (5 maxcon words,
  // first written by the iterations below) and the head of the Hessian region (>= 6 + 10 nbody + 6 nv >= 3 maxcon words in every
  // layout; dead between the qacc_smooth solve and the first factorisation).
  contact_Jx3<TREE ? 8 : 16>(c, x, S(asmo), S(qvel), c.L.cp, c.L.cW, c.L.H);
  for (int r = lane; r < nrow; r += WAVE) {
    const double a = -S(aref)[r] * row_Jx_at(c, c.L.H, r) - S(jar)[r];   // aref = -B efc_vel - K imp (pos - margin): make_constraint parked B in aref, the K term in jar
    S(aref)[r] = a;
    S(jar)[r] = row_Jx(c, r) - a;
  }
  SYNC();
  double xi = lane < nv ? x[lane] : 0.0;
  double cost_ws = solver_cost_part(c, Ma, xi);   // both costs: the lanes' shares first, then the two wave sums together
  double jsm[RPL];
  double csm = 0;
  {
    const LimRows q = lim_rows(c);
    const double xs = lane < nv ? S(asmo)[lane] : 0.0, j0 = xs - q.A0, j1 = -xs - q.A1;
    if (j0 < 0) csm += 0.5 * q.D0 * j0 * j0;
    if (j1 < 0) csm += 0.5 * q.D1 * j1 * j1;
  }
#pragma unroll
  for (int q = 0; q < RPL; q++) {
    int r = lane + WAVE * q;
    double jv = r < nrow ? row_Jx_at(c, c.L.cW, r) - S(aref)[r] : 1.0;
    jsm[q] = jv;
    if (jv < 0) csm += 0.5 * S(D)[r >> 2] * jv * jv;
  }
  double cost_sm = csm;
  wave_sum2(cost_ws, cost_sm);
  double cost = cost_ws;
  if (cost_ws > cost_sm) {
    if (lane < nv) { xi = S(asmo)[lane]; x[lane] = xi; }
#pragma unroll
    for (int q = 0; q < RPL; q++) { int r = lane + WAVE * q; if (r < nrow) S(jar)[r] = jsm[q]; }
    SYNC();
    Ma = dense_Mx(c, x);
    cost = solver_cost(c, Ma, xi);
  }
  int iters = 0;
  // loop invariants of this lane's dof, kept in registers: its limit rows, smooth force and unconstrained acceleration
  const LimRows lq = lim_rows(c);
  // (unconditional loads at a clamped index + selects: no predicated region right in front of the iteration loop -- the register
  // allocator parked loop-invariant registers of the step loop in exactly such a region once, see tools/exec_copy_check.py)
  double qsm_i = S(qsm)[lane < nv ? lane : 0], asmo_i = S(asmo)[lane < nv ? lane : 0];
  asm volatile("" : "+v"(qsm_i), "+v"(asmo_i));
  qsm_i = lane < nv ? qsm_i : 0.0; asmo_i = lane < nv ? asmo_i : 0.0;
  PROF(11);
  for (int iter = 0; iter < maxiter; iter++) {
    iters++;
    // ---- per-contact force / weight summaries of the active set
    for (int ci = lane; ci < ncon; ci += WAVE) {
      double mu = S(cpar)[ci], f[4], dact[4];
      const double Dr = S(D)[ci];
      for (int k = 0; k < 4; k++) {
        double j = S(jar)[4 * ci + k];
        dact[k] = j < 0 ? Dr : 0.0;
        f[k] = j < 0 ? -Dr * j : 0.0;
      }
      double* cp = S(cp) + 3 * ci;
      cp[0] = ((f[0] + f[1]) + f[2]) + f[3];
      cp[1] = mu * (f[0] - f[1]);
      cp[2] = mu * (f[2] - f[3]);
      double* W = S(cW) + 5 * ci;
      W[0] = ((dact[0] + dact[1]) + dact[2]) + dact[3];
      W[1] = mu * (dact[0] - dact[1]);
      W[2] = mu * (dact[2] - dact[3]);
      W[3] = mu * mu * (dact[0] + dact[1]);
      W[4] = mu * mu * (dact[2] + dact[3]);
    }
    SYNC();
    // ---- gradient: own limit rows (lane-local) + dof-major gather of J^T f over the contacts touching the dof
    double g = 0, dl = 0;
    if (lane < nv) {
      double qc = 0;
      const double j0 = xi - lq.A0, j1 = -xi - lq.A1;
      if (j0 < 0) { qc -= lq.D0 * j0; dl += lq.D0; }   // force -D jar through the row +e_dof
      if (j1 < 0) { qc += lq.D1 * j1; dl += lq.D1; }   // row -e_dof
      if constexpr (TREE) {
        // one moving body per contact: its block is 3 x 8 at 24 ci (make_constraint) and this dof's slot is its chain position -- no
        // slot byte, no info word, no branch
        const double* Js = S(Jb) + role_d_pos(c);
        for (unsigned long long mk = ((const unsigned long long*)S(cmask))[lane]; mk; mk &= mk - 1) {
          const int ci = __builtin_ctzll(mk);
          const double* Jb = Js + 24 * ci;
          const double* cp = S(cp) + 3 * ci;
          qc += Jb[0] * cp[0] + Jb[8] * cp[1] + Jb[16] * cp[2];
        }
      } else {
        for (unsigned long long mk = ((const unsigned long long*)S(cmask))[lane]; mk; mk &= mk - 1) {
          int ci = __builtin_ctzll(mk);
          const int s = SLOT_OF(ci, lane, role_d_pos(c));
          const int info = (c.si + c.L.con_b)[4 * ci + 3], ns = (info >> 20) ? 16 : 8;
          const double* Jb = S(Jb) + (info & 0xFFFFF);
          const double* cp = S(cp) + 3 * ci;
          qc += Jb[s] * cp[0] + Jb[ns + s] * cp[1] + Jb[2 * ns + s] * cp[2];
        }
      }
      g = Ma - qsm_i - qc;
      if (!TREE) S(dlim)[lane] = dl;
    }
    double gn = wave_sum(g * g);
    PROF(12);
    if (gn <= c.P->grad_thresh) break;   // scale * sqrt(gn) < tol  <=>  gn <= grad_thresh (grad_threshold on the host: the last double that passes)
    SYNC();
    // ---- Hessian H = M + J^T diag(D_active) J, lower triangle: entry-major gather (every lane a few entries).
    // All loads of the mass-matrix / mask words are issued before any store so they pipeline.
    if (!TREE) {
      const unsigned long long* cm = (const unsigned long long*)S(cmask);
      double hreg[C::EPL];
      unsigned long long mreg[C::EPL];
      // (the entry words are made opaque here so that the addresses derived from them are computed in this rarely taken
      // block instead of being hoisted to kernel entry and kept in registers / scratch for the whole launch)
      unsigned ent[C::EPL];
      int pi[C::EPL], pj[C::EPL];   // chain positions of the entry's two dofs (slot lookup, SLOT_OF)
#pragma unroll
      for (int m = 0; m < C::EPL; m++) {
        unsigned w = (unsigned)pt_global(launder_ptr(c.P->aux.ai + c.P->aux.o_ent))[c.lane + WAVE * m];   // loaded here, in the rarely taken block
        ent[m] = w & 0xFFFFu;
        pi[m] = (w >> 16) & 0xF; pj[m] = (w >> 20) & 0xF;
      }
#pragma unroll
      for (int m = 0; m < C::EPL; m++) {
        unsigned e = ent[m];
        int i = e == 0xFFFFu ? 0 : (int)(e >> 8), jj = e == 0xFFFFu ? 0 : (int)(e & 0xFF);
        double h = SAME_TREE(i, jj) ? S(M)[MIDX(i, jj)] : 0.0;
        if (i == jj) h += S(dlim)[i];
        hreg[m] = h;
        mreg[m] = e == 0xFFFFu ? 0ull : (cm[i] & cm[jj]);
      }
#pragma unroll
      for (int m = 0; m < C::EPL; m++) {
        unsigned e = ent[m];
        int i = e >> 8, jj = e & 0xFF;
        double h = hreg[m];
        for (unsigned long long mk = mreg[m]; mk; mk &= mk - 1) {
          int ci = __builtin_ctzll(mk);
          const int si = SLOT_OF(ci, i, pi[m]), sj = SLOT_OF(ci, jj, pj[m]);
          const int info = (c.si + c.L.con_b)[4 * ci + 3], ns = (info >> 20) ? 16 : 8;
          const double* Jb = S(Jb) + (info & 0xFFFFF);
          const double* W = S(cW) + 5 * ci;
          double a0 = Jb[si], a1 = Jb[ns + si], a2 = Jb[2 * ns + si], b0 = Jb[sj], b1 = Jb[ns + sj], b2 = Jb[2 * ns + sj];
          h += a0 * (W[0] * b0 + W[1] * b1 + W[2] * b2) + a1 * (W[1] * b0 + W[3] * b1) + a2 * (W[2] * b0 + W[4] * b2);
        }
        hreg[m] = h;
      }
#pragma unroll
      for (int m = 0; m < C::EPL; m++) {
        unsigned e = ent[m];
        if (e != 0xFFFFu) S(H)[HP((int)(e >> 8), (int)(e & 0xFF))] = hreg[m];
      }
    }
    SYNC();
    PROF(13);
    int hfail;
    double sr;
    if (TREE) {  // every contact touches one moving body: H keeps the tree sparsity of M (see tree_factor_solve)
      double row[8];
      tree_rows(c, row, dl, ncon > 0);
      sr = -tree_factor_solve(c, row, g, &hfail);
    } else {
      sr = -ldl_solve_rows(c, S(H), S(H), g, &hfail);
    }
    if (hfail) break;
    if (lane < nv) S(search)[lane] = sr;
    SYNC();
    PROF(14);
    // ---- exact line search
    double Mv = dense_Mx(c, S(search));
    contact_Jx<TREE ? 8 : 16>(c, S(search));
    // each lane keeps its contact rows (r = lane + 64 q) and its dof's two limit rows (jar, Jv, D) in registers
    double rj[RPL + 2], rjv[RPL + 2], rD[RPL + 2];
#pragma unroll
    for (int q = 0; q < RPL; q++) {
      int r = lane + WAVE * q;
      bool ok = r < nrow;
      rjv[q] = ok ? row_Jx(c, r) : 0.0;
      rj[q] = ok ? S(jar)[r] : 1.0;      // absent rows: jar > 0 and Jv = 0 never contribute
      rD[q] = ok ? S(D)[r >> 2] : 0.0;
    }
    rj[RPL] = xi - lq.A0; rjv[RPL] = sr; rD[RPL] = lq.D0;
    rj[RPL + 1] = -xi - lq.A1; rjv[RPL + 1] = -sr; rD[RPL + 1] = lq.D1;
    double g1 = lane < nv ? sr * (Ma - qsm_i) : 0.0, g2 = lane < nv ? sr * Mv : 0.0;
    double alpha = 0, lo = 0, hi = -1, d0 = 0, f1, f2;
    auto ls_terms = [&]() {   // this lane's share of the constraint terms of the derivatives at alpha
      f1 = 0; f2 = 0;
#pragma unroll
      for (int q = 0; q < RPL + 2; q++) {
        double j = rj[q] + alpha * rjv[q];
        if (j < 0) { f1 += rD[q] * j * rjv[q]; f2 += rD[q] * rjv[q] * rjv[q]; }
      }
    };
    ls_terms();   // the first evaluation (alpha == 0) is ready with g1 and g2: the four wave sums run together
    wave_sum4(g1, g2, f1, f2);
    for (int ls = 0;;) {
      f1 += g1 + alpha * g2;
      f2 += g2;
      if (ls == 0) d0 = fabs(f1);
      if (fabs(f1) <= 1e-10 * d0) break;
      if (f1 < 0) lo = alpha; else hi = alpha;
      double an = alpha - f1 * fast_rcp(f2);
      if (an <= lo || (hi >= 0 && an >= hi)) an = hi >= 0 ? 0.5 * (lo + hi) : 2 * (alpha > 0 ? alpha : 1.0);
      alpha = an;
      if (++ls == 50) break;
      ls_terms();
      wave_sum2(f1, f2);
    }
    PROF(15);
    if (alpha == 0) break;
    if (lane < nv) { xi += alpha * sr; x[lane] = xi; Ma += alpha * Mv; }
#pragma unroll
    for (int q = 0; q < RPL; q++) {
      int r = lane + WAVE * q;
      if (r < nrow) S(jar)[r] = rj[q] + alpha * rjv[q];
    }
    SYNC();
    double oldcost = cost;
    {  // cost at the new point from the rows this lane already holds (same terms as solver_cost, no LDS round trip)
      double v = lane < nv ? 0.5 * (Ma - qsm_i) * (xi - asmo_i) : 0.0;
      const double j0 = xi - lq.A0, j1 = -xi - lq.A1;
      if (j0 < 0) v += 0.5 * lq.D0 * j0 * j0;
      if (j1 < 0) v += 0.5 * lq.D1 * j1 * j1;
#pragma unroll
      for (int q = 0; q < RPL; q++) { const double jn = rj[q] + alpha * rjv[q]; if (jn < 0) v += 0.5 * rD[q] * jn * jn; }
      cost = wave_sum(v);
    }
    if (scale * (oldcost - cost) < tol) break;
  }
  c.st_newton += iters;
  if (iters > c.st_maxnewton) c.st_maxnewton = iters;
  SYNC();
}

#ifdef SUMO_DBG_DUMP
#define DUMP(slot, ptr, n) do { if (c.dbg && c.st_forward <= 20 && c.lane < (n)) c.dbg[((c.st_forward - 1) * 8 + (slot)) * 64 + c.lane] = (ptr)[c.lane]; } while (0)
#else
#define DUMP(slot, ptr, n) do { } while (0)
#endif
// ---- mj_forward ----------------------------------------------------------------------------------------------
template <class C>
__device__ __forceinline__ void forward(C& c) {
  const auto& mdl = model_view(c);
  const int lane = c.lane, nv = mdl.nv;
  c.st_forward++;
  DUMP(0, S(qpos), mdl.nq); DUMP(1, S(qvel), nv); DUMP(2, S(ctrl), mdl.nu); DUMP(7, S(warm), nv);
  position_velocity(c);
  collision(c);
  make_constraint(c);
#ifdef SUMO_DBG_DUMP
  if (c.dbg && c.st_forward <= 20 && lane < 3) c.dbg[((c.st_forward - 1) * 8 + 5) * 64 + lane] = lane == 0 ? c.ncon : (lane == 1 ? c.nefc : c.nlim);
#endif
  // (efc_vel and aref: newton_solve forms them in its set-up pass; until then B and K*imp*(pos-margin) stay parked in aref / jar,
  // and nothing in between touches them, qvel, Jb or the dof indices)
  PROF(8);
  mass_matrix(c);  // last user of the kinematic scratch; H may overwrite it from here on
  PROF(9);
  // smooth forces: passive (damping) - bias + actuation
  KCONSTS();
  if (lane < nv) S(qsm)[lane] = -K.d_damp * S(qvel)[lane] - S(bias)[lane];
  SYNC();
  if (lane < mdl.nu) {
    double u = S(ctrl)[lane];
    if (u < K.a_lo) u = K.a_lo;
    if (u > K.a_hi) u = K.a_hi;
    S(qsm)[K.a_dof] += K.a_gear * u;  // one motor per dof in these scenes
  }
  SYNC();
  DUMP(3, S(qsm), nv);
  // qacc_smooth = M^-1 qfrc_smooth
  int mfail;
  double as;
  if (c.L.tree_ok) {
    double row[8];
    tree_rows(c, row, 0.0, false);
    as = tree_factor_solve(c, row, lane < nv ? S(qsm)[lane] : 0.0, &mfail);
  } else {  // unknown tree shape: pack M into the Hessian buffer and use the dense factorisation
#pragma unroll
    for (int m = 0; m < C::EPL; m++) {
      unsigned e = (unsigned)pt_global(launder_ptr(c.P->aux.ai + c.P->aux.o_ent))[c.lane + WAVE * m];   // (address arithmetic stays in this rarely taken block)
      e &= 0xFFFFu;
      if (e != 0xFFFFu) { int i = e >> 8, jj = e & 0xFF; S(H)[HP(i, jj)] = SAME_TREE(i, jj) ? S(M)[MIDX(i, jj)] : 0.0; }
    }
    SYNC();
    as = ldl_solve_rows(c, S(H), S(H), lane < nv ? S(qsm)[lane] : 0.0, &mfail);
  }
  if (mfail) as = 0.0;
  if (lane < nv) S(asmo)[lane] = as;
  SYNC();
  PROF(10);
  DUMP(4, S(asmo), nv);
  if (c.htree) newton_solve<true>(c);
  else {
    // The general (dense-factorisation) path costs ~1.65x a tree-path forward and the envs on it -- agents in contact with each
    // other, a few per launch -- are the stragglers every launch waits for (tools/slot_trace.py).  From its first dense
    // forward on, such a wave issues ahead of the wave it shares the SIMD with (which has slack).
    __builtin_amdgcn_s_setprio(3);
    newton_solve<false>(c);
    c.st_dense++;
    if (c.hcross) c.st_cross++;
  }
  PROF(16);
  DUMP(6, S(x), nv);
  c.st_ncon += c.ncon;
  c.st_nefc += c.nefc;
  if (c.ncon > c.st_maxcon) c.st_maxcon = c.ncon;
  if (c.nefc > c.st_maxefc) c.st_maxefc = c.nefc;
  c.st_dropped += c.ndropped;
}

// qpos '+'= h * vel  (vel in LDS), one lane per joint
template <class C>
__device__ __forceinline__ void integrate_pos(C& c, double* qpos, const double* vel, double h) {
  if (c.lane < c.P->mdl.njnt) {
    const int qa = role_jt_qadr(c), da = role_jt_dadr(c);
    if (!role_jt_hinge(c)) {
      for (int k = 0; k < 3; k++) qpos[qa + k] += h * vel[da + k];
      double ax[3] = {vel[da + 3], vel[da + 4], vel[da + 5]}, qr[4], q[4] = {qpos[qa + 3], qpos[qa + 4], qpos[qa + 5], qpos[qa + 6]};
      double ang = h * normalize3(ax);
      axisangle2quat(qr, ax, ang);
      normalize4(q);
      mulquat(q, q, qr);
      qpos[qa + 3] = q[0]; qpos[qa + 4] = q[1]; qpos[qa + 5] = q[2]; qpos[qa + 6] = q[3];
    } else {
      qpos[qa] += h * vel[da];
    }
  }
}

// frame_skip x mj_step with the RK4 stages flattened into one loop, so forward() has a single (inlined) call site.
// MuJoCo's bad-value test (mj_checkPos / mj_checkVel / mj_checkAcc: NaN or |x| > mjMAXVAL = 1e10 in qpos, qvel, qacc; the
// reference turns the resulting warning into a MujocoException, mujoco-py/mujoco_py/builder.py:351-369).  Wave-uniform result.
template <class C>
__device__ __forceinline__ int state_is_bad(C& c) {
  const auto& mdl = model_view(c);
  const int lane = c.lane;
  bool bad = false;
  for (int i = lane; i < mdl.nq; i += WAVE) bad |= !(fabs(S(qpos)[i]) <= 1e10);   // NaN fails the comparison too
  for (int i = lane; i < mdl.nv; i += WAVE) bad |= !(fabs(S(qvel)[i]) <= 1e10) || !(fabs(S(warm)[i]) <= 1e10);
  return __builtin_amdgcn_ballot_w64(bad) != 0ull;
}

// RK4 tableau (MuJoCo): A = diag(1/2, 1/2, 1), B = (1/6, 1/3, 1/3, 1/6); the warm start saved at the end of a step is
// the last stage's qacc.
template <class C>
__device__ __forceinline__ void mj_steps(C& c, int nsteps) {
  const auto& mdl = model_view(c);
  const int lane = c.lane, nq = mdl.nq, nv = mdl.nv;
  const double h = MF(opt)[SUMO_OPT_TIMESTEP];
  double q0 = 0, v0 = 0, accv = 0, acca = 0;   // this lane's entry of the step's start state and of the RK4 accumulators
  for (int sub = 0; sub < 4 * nsteps; sub++) {
    const int stage = sub & 3;
    c.use_prev = (c.L.warm_mode == 1 && stage != 0) ? 1 : 0;
    // make the lane id opaque per iteration: stops the compiler from hoisting hundreds of lane-dependent address
    // computations out of this loop (they would be spilled to scratch under the 256-register budget)
    asm volatile("" : "+v"(c.lane));
    forward(c);
    if (stage == 0) {
      if (lane < nq) q0 = S(qpos)[lane];
      if (lane < nv) {
        v0 = S(qvel)[lane];
        accv = 0.0 + (1.0 / 6.0) * S(qvel)[lane];
        acca = 0.0 + (1.0 / 6.0) * S(x)[lane];
      }
    } else {
      const double Bi = stage == 3 ? 1.0 / 6.0 : 1.0 / 3.0;
      if (lane < nv) { accv += Bi * S(qvel)[lane]; acca += Bi * S(x)[lane]; }
    }
    SYNC();
    if (stage < 3) {
      const double Ai = stage == 2 ? 1.0 : 0.5;  // A[stage]
      double dv = 0;
      if (lane < nv) { S(tmpv)[lane] = Ai * S(qvel)[lane]; dv = Ai * S(x)[lane]; }
      if (lane < nq) S(qpos)[lane] = q0;
      SYNC();
      integrate_pos(c, S(qpos), S(tmpv), h);
      if (lane < nv) S(qvel)[lane] = v0 + h * dv;
      SYNC();
    } else {
      if (lane < nq) S(qpos)[lane] = q0;
      if (lane < nv) { S(qvel)[lane] = v0 + h * acca; S(warm)[lane] = S(x)[lane]; S(tmpv)[lane] = accv; }
      SYNC();
      integrate_pos(c, S(qpos), S(tmpv), h);
      SYNC();
    }
  }
}

// ---- RNG / reset / observation -----------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32(uint32_t* out, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ double rng_uniform(uint64_t seed, uint32_t reset_count, uint32_t k) {
  uint32_t o[4];
  philox4x32(o, reset_count, k >> 1, 0u, 0x53554D4Fu, (uint32_t)seed, (uint32_t)(seed >> 32));
  uint32_t a = ((k & 1) ? o[2] : o[0]) >> 5, b = ((k & 1) ? o[3] : o[1]) >> 6;
  return (a * 67108864.0 + b) / 9007199254740992.0;
}

// sumo.py:232-253 with a counter RNG; state ends up in LDS (qpos, qvel, warm)
template <class C>
__device__ __forceinline__ void reset_state(C& c, uint64_t seed, uint32_t rc) {
  const auto& mdl = model_view(c);
  const int lane = c.lane, nq = mdl.nq, nv = mdl.nv;
  if (lane < nq) S(qpos)[lane] = MF(qpos0)[lane];
  SYNC();
  if (lane < mdl.nagent) {
    double phi = 2.0 * PI_D * rng_uniform(seed, rc, 0);
    double ang = phi + lane * (2.0 * PI_D / 2.0);
    int qa = MI(agent_qposadr)[lane];
    S(qpos)[qa] = 1.15 * slow_cos(ang);
    S(qpos)[qa + 1] = 1.15 * slow_sin(ang);
    S(qpos)[qa + 2] = 1.25;
  }
  SYNC();
  if (lane < nq) S(qpos)[lane] += -0.1 + 0.2 * rng_uniform(seed, rc, 1 + lane);
  if (lane < nv) {
    double u1 = rng_uniform(seed, rc, RNG_NORMAL_BASE + 2 * (lane >> 1));
    double u2 = rng_uniform(seed, rc, RNG_NORMAL_BASE + 2 * (lane >> 1) + 1);
    double rr = sqrt(-2.0 * slow_log(1.0 - u1));
    double z = (lane & 1) ? rr * slow_sin(2.0 * PI_D * u2) : rr * slow_cos(2.0 * PI_D * u2);
    S(qvel)[lane] = 0.1 * z;
    S(warm)[lane] = 0.0;
  }
  SYNC();
  if (lane < mdl.njnt && MI(jnt_type)[lane] == SUMO_JNT_FREE) {
    double* q = S(qpos) + MI(jnt_qposadr)[lane] + 3;
    double qq[4] = {q[0], q[1], q[2], q[3]};
    normalize4(qq);
    q[0] = qq[0]; q[1] = qq[1]; q[2] = qq[2]; q[3] = qq[3];
  }
  SYNC();
}

// agents.py:190-214 (cfrc_ext == 0) + time feature (sumo_env.py:68-70)
// ---- coherent hand-over accessors -----------------------------------------------------------------------------------
// In the fused rollout launch an env moves between waves (possibly on another XCD, whose L2 is not coherent with ours) from one
// step to the next.  Only a few hundred bytes cross: the state record, the counters, the observations and the done flags.
// They are written and read with agent-scope relaxed atomics -- `sc1` stores that write through to memory and `sc1` loads
// that bypass the non-coherent cache levels (MI355X_MICROARCH.md, inter-workgroup visibility, the all-sc1 form) -- so no
// L2 write-back / invalidate fence is needed per step: a release fence there flushes every dirty line of the XCD's L2,
// scratch frames included, 2 million times a second (measured: 67 KB of HBM writes per env step against 2.5 KB algorithmic).
// COH = false (per-step launch): plain accesses, the kernel boundary orders them.
// (through global-address-space pointers: in the rollout kernel the buffers' addresses come out of the laundered launch arguments,
// i.e. generic pointers, whose flat accesses would tie up the LDS counter as well -- see PT_GAS in ppo_tile.h)
template <bool COH, class T>
__device__ __forceinline__ T hand_load(const T* p) {
  if (COH) return __hip_atomic_load(pt_global(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *pt_global(p);
}
template <bool COH, class T>
__device__ __forceinline__ void hand_store(T* p, T v) {
  if (COH) __hip_atomic_store(pt_global(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *pt_global(p) = v;
}

template <bool COH = false, class C>
__device__ __forceinline__ void write_obs(C& c, float* obs, int obs_stride, int num_steps) {
  const auto& mdl = model_view(c);
  const double adjz = c.P->adjust_z;
  for (int idx = c.lane; idx < 2 * obs_stride; idx += WAVE) {
    int a = idx >= obs_stride, k = idx - a * obs_stride, o = 1 - a;
    int nqa = MI(agent_nq)[a], nva = MI(agent_nv)[a], nba = MI(agent_nbody)[a];
    int dim = nqa + nva + 6 * nba + 14;
    float v = 0.0f;
    // get_qpos() adds _adjust_z to the z entry of the copy it returns (agents.py:155-161): own z and the opponent's z
    if (k < nqa) { double q = S(qpos)[MI(agent_qposadr)[a] + k]; if (k == 2) q += adjz; v = (float)q; }
    else if (k < nqa + nva) v = (float)S(qvel)[MI(agent_dofadr)[a] + (k - nqa)];
    else if (k < nqa + nva + 6 * nba) v = 0.0f;
    else if (k < nqa + nva + 6 * nba + 7) { const int j = k - nqa - nva - 6 * nba; double q = S(qpos)[MI(agent_qposadr)[o] + j]; if (j == 2) q += adjz; v = (float)q; }
    else if (k < dim - 1) v = 0.0f;
    else if (k == dim - 1) v = (float)(-1.0 + 2.0 * num_steps / 500.0);
    hand_store<COH>(obs + idx, v);
  }
}

__device__ __forceinline__ float sumsq_f32(const float* a, int n) {  // numpy float32 pairwise sum of squares (n < 128)
  if (n < 8) { float r = 0.0f; for (int i = 0; i < n; i++) r += a[i] * a[i]; return r; }
  float r[8];
  for (int j = 0; j < 8; j++) r[j] = a[j] * a[j];
  int i;
  for (i = 8; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; j++) r[j] += a[i + j] * a[i + j];
  float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; i++) res += a[i] * a[i];
  return res;
}

// the same sum over the step's control vector in LDS (S(ctrl)[i] == (double)action[i] exactly: float -> double -> float)
__device__ __forceinline__ float sumsq_f32_ctrl(const double* u, int n) {
  if (n < 8) { float r = 0.0f; for (int i = 0; i < n; i++) { const float a = (float)u[i]; r += a * a; } return r; }
  float r[8];
  for (int j = 0; j < 8; j++) { const float a = (float)u[j]; r[j] = a * a; }
  int i;
  for (i = 8; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; j++) { const float a = (float)u[i + j]; r[j] += a * a; }
  float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; i++) { const float a = (float)u[i]; res += a * a; }
  return res;
}

template <class C>
__device__ __forceinline__ void ctx_init(C& c, const Params* P, double* smem) {
  c.P = P;
  if constexpr (std::is_same<typename C::LT, Layout>::value) c.L = P->L;
  c.sm = smem;
  c.si = (int*)(smem + c.L.i_base);
  c.sb = (unsigned char*)(smem + c.L.i_base);
  c.lane = threadIdx.x;
  c.kp = P->lanes + c.lane;
  c.prp = P->pair_rec + c.lane;
  c.pbp = P->pair_bound + c.lane;
  // static tables -> LDS (once per launch); world centres into the tail of xipos / gaxis
#if SUMO_STAT_LDS
  for (int i = c.lane; i < P->aux.n_stat_d; i += WAVE) smem[P->L.stat_d + i] = P->aux.af[P->aux.o_stat_d + i];
  for (int i = c.lane; i < P->aux.n_stat_i; i += WAVE) c.si[P->L.stat_i + i] = P->aux.ai[P->aux.o_stat_i + i];
#endif
  {
    const int nb = P->mdl.nbody, nw = P->aux.nworld, nc = P->aux.nc;
    const double* wpos = P->aux.af + P->aux.o_wpa;
    for (int i = c.lane; i < 3 * nw; i += WAVE) { smem[P->L.xipos + 3 * nb + i] = wpos[i]; smem[P->L.gaxis + 3 * nb + i] = wpos[3 * nw + i]; }
  }
  c.role0 = P->lanes[c.lane].role0;
  c.role1 = P->lanes[c.lane].role1;
  __syncthreads();
  c.ncon = c.nlim = c.nefc = c.ndropped = c.use_prev = 0;
  c.st_forward = c.st_newton = c.st_ncon = c.st_nefc = c.st_maxcon = c.st_maxefc = c.st_maxnewton = c.st_dropped = c.st_dense = c.st_cross = 0;
  c.st_diverged = 0;
  c.st_cb3 = c.st_rodcap = 0;
#ifdef SUMO_PROFILE
  for (int k = 0; k < 24; k++) c.prof[k] = 0;
  c.tprev = clock64();
#endif
}
// Checksum of a state record as it crosses between waves in the fused rollout launch (COH): every word is mixed with its index,
// the lanes' contributions are summed over the wave.  The writer stores it next to the record's sequence tag (counters[2..3]),
// the wave that takes the env over recomputes it from what it LOADED: a stale or torn read of the record -- the failure the
// hand-rolled sc1 protocol would produce silently -- raises the launch's abort flag instead (sumo_rollout_status).
__device__ __forceinline__ unsigned rec_hash(double v, int i) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  return (lo ^ (hi * 0x9E3779B1u)) * 0x85EBCA77u + (unsigned)(i + 1) * 0xC2B2AE3Du;
}
__device__ __forceinline__ unsigned wave_usum(unsigned v) {   // wave_sum's stages on an integer; only lane 63 is read
  int x = (int)v;
#define WAVE_SUM_STAGE(CTRL) x += __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
  WAVE_SUM_STAGES(WAVE_SUM_STAGE)
#undef WAVE_SUM_STAGE
  return (unsigned)__builtin_amdgcn_readlane(x, 63);
}
template <bool COH = false, class C, class SA>   // SA: StepArgs by value (per-step kernel) or in the kernel-argument segment (rollout kernel)
__device__ __forceinline__ unsigned load_state(C& c, const SA& a, int e) {   // returns the record's checksum (COH) or 0
  const int nq = c.P->mdl.nq, nv = c.P->mdl.nv, lane = c.lane;
  const double* st = a.state + (size_t)e * a.state_stride;
  unsigned h = 0;
  for (int i = lane; i < nq + 2 * nv; i += WAVE) {
    double v = hand_load<COH>(st + i);
    if (COH) h += rec_hash(v, i);
    if (i < nq) S(qpos)[i] = v; else if (i < nq + nv) S(qvel)[i - nq] = v; else S(warm)[i - nq - nv] = v;
  }
  return COH ? wave_usum(h) : 0u;
}
template <bool COH = false, class C, class SA>
__device__ __forceinline__ unsigned store_state(C& c, const SA& a, int e) {
  const int nq = c.P->mdl.nq, nv = c.P->mdl.nv, lane = c.lane;
  double* st = a.state + (size_t)e * a.state_stride;
  unsigned h = 0;
  for (int i = lane; i < nq + 2 * nv; i += WAVE) {
    const double v = i < nq ? S(qpos)[i] : (i < nq + nv ? S(qvel)[i - nq] : S(warm)[i - nq - nv]);
    if (COH) h += rec_hash(v, i);
    hand_store<COH>(st + i, v);
  }
  return COH ? wave_usum(h) : 0u;
}
template <class C>
__device__ __forceinline__ void flush_stats(C& c, unsigned long long* stats) {
  if (c.lane == 0 && stats) {
    atomicAdd(stats + 0, (unsigned long long)c.st_forward);
    atomicAdd(stats + 1, (unsigned long long)c.st_newton);
    atomicAdd(stats + 2, (unsigned long long)c.st_ncon);
    atomicAdd(stats + 3, (unsigned long long)c.st_nefc);
    atomicMax(stats + 4, (unsigned long long)c.st_maxcon);
    atomicMax(stats + 5, (unsigned long long)c.st_maxefc);
    atomicMax(stats + 6, (unsigned long long)c.st_maxnewton);
    atomicAdd(stats + 7, (unsigned long long)c.st_dropped);
    if (c.st_diverged) atomicAdd(stats + 8, (unsigned long long)c.st_diverged);
    if (c.st_cb3) atomicAdd(stats + 11, (unsigned long long)c.st_cb3);
    if (c.st_rodcap) atomicAdd(stats + 12, (unsigned long long)c.st_rodcap);
#ifdef SUMO_PROFILE
    for (int k = 0; k < 24; k++) atomicAdd(stats + 16 + k, c.prof[k]);
#endif
  }
}

// ---------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------
// Longest-first schedule for small launches: perm[rank] = env, rank = number of envs with a larger (cost, -index) key --
// the same order as a stable descending sort.  Run by the first workgroups of the step launch itself (on the estimates
// of the PREVIOUS launch, for the NEXT one), so no kernel sits between two env steps of a group for it: a library sort
// there cost 136 us on average (its large workgroups wait until the other group's whole launch has been placed), a
// separate rank kernel still 35-40 us.
#define SCHED_RANK_MAX 4096
__device__ __forceinline__ void sched_rank(const int* __restrict__ cost, int n, int* __restrict__ perm, int block, int lane) {
  const int e = block * WAVE + lane;
  const int mine = e < n ? ((cost[e] << 12) | (SCHED_RANK_MAX - 1 - e)) : 0x7FFFFFFF;
  int rank = 0;
  for (int j0 = 0; j0 < n; j0 += 8 * WAVE) {   // 512 keys per batch: eight coalesced loads in flight, then lane broadcasts
    int key[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int j = j0 + WAVE * u + lane;
      key[u] = j < n ? ((cost[j] << 12) | (SCHED_RANK_MAX - 1 - j)) : -1;
    }
#pragma unroll
    for (int u = 0; u < 8; u++)
#pragma unroll 8
      for (int l = 0; l < WAVE; l++) rank += (__builtin_amdgcn_readlane(key[u], l) > mine) ? 1 : 0;
  }
  if (e < n) perm[rank] = e;
}

extern __shared__ double smem_dyn[];
#ifdef SUMO_DBG_POISON_LDS
// development: every LDS word holds a signalling pattern before an env step starts, so that a phase that reads a word nobody
// wrote shows up as NaN in the parity tests instead of depending on what the previous step / workgroup left there
__device__ __forceinline__ void poison_lds(const Params* P, int lane) {
  const int n = P->L.total_bytes / 8;
#ifndef SUMO_DBG_POISON_LO
#define SUMO_DBG_POISON_LO 0
#define SUMO_DBG_POISON_HI 0x7fffffff
#endif
  // kinds 4 / 5: PLAUSIBLE leftovers -- what another env's step would leave in the slot: doubles of order one (kind 4) or pairs of
  // small integers (kind 5), different in every word and workgroup (uniform patterns hide reads that are compared or used as masks);
  // LO / HI restrict the fill to a range of 8-byte words (bisection)
  for (int i = lane; i < n; i += WAVE) {
    if (i < SUMO_DBG_POISON_LO || i >= SUMO_DBG_POISON_HI) continue;
    unsigned h = (unsigned)i * 2654435761u + (unsigned)blockIdx.x * 40503u + 12345u;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    double v = 0.0;
    if (SUMO_DBG_POISON_LDS == 1) v = 1e300;
    else if (SUMO_DBG_POISON_LDS == 2) v = __longlong_as_double(0x7FF8DEADBEEF0000ll);
    else if (SUMO_DBG_POISON_LDS == 4) v = ((double)(h & 0xFFFFFu) / 524288.0 - 1.0) * 1.5;
    else if (SUMO_DBG_POISON_LDS == 5) v = __longlong_as_double((long long)(h % 24u) | ((long long)((h >> 8) % 24u) << 32));
    smem_dyn[i] = v;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  {   // what ctx_init keeps in LDS for the whole launch: the world geoms' centres / axes
    const int nb = P->mdl.nbody, nw = P->aux.nworld;
    const double* wpos = P->aux.af + P->aux.o_wpa;
    for (int i = lane; i < 3 * nw; i += WAVE) { smem_dyn[P->L.xipos + 3 * nb + i] = wpos[i]; smem_dyn[P->L.gaxis + 3 * nb + i] = wpos[3 * nw + i]; }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
#endif

// One env step of env `e` by this wave: state record -> LDS, frame_skip x RK4 mj_step, game rules, rewards, done, auto-reset,
// observation write, state record back (the whole of SumoEnv._step + the wrappers + the worker's auto-reset:
// sumo.py:120-202, sumo_env.py:40-72, monitor.py:51-78, subproc_vec_env.py:10-19).  Shared by the per-step launch
// (sumo_step_kernel) and the fused multi-step rollout launch (sumo_rollout_kernel).
template <bool COH = false, class C, class SA>
__device__ __forceinline__ void env_step_body(C& c, const SA& a, int e) {
  const auto& mdl = model_view(c);
  const int lane = c.lane;
  if (a.trace && lane == 0) a.trace[4 * e] = wall_clock64();
  const unsigned rec_sum = load_state<COH>(c, a, e);
#ifndef SUMO_NO_HANDCHECK
  if (COH) {   // fused rollout: the record must be the one the env's previous step of THIS launch published (tag and checksum)
    const int k0 = ((const int*)(S(stash) + 4))[1];   // parked by the ticket loop
    if (k0 > 0) {
      const int* cn = a.counters + 4 * e;
      const int tag = hand_load<true>(cn + 2);
      const unsigned chk = (unsigned)hand_load<true>(cn + 3);
      if ((tag != a.seq_base + k0 || chk != rec_sum) && lane == 0) {
        __hip_atomic_store(pt_global(a.abort_flag), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a.stats) atomicAdd(a.stats + 10, 1ull);
      }
    }
  }
#endif
#ifdef SUMO_DBG_RELOAD_CTRL
  if (COH && lane < mdl.nu) {
    const float* act0 = a.actions + (size_t)e * 2 * a.act_stride;
    int ag = lane >= MI(agent_uadr)[1] ? 1 : 0;
    S(ctrl)[lane] = (double)hand_load<true>(act0 + ag * a.act_stride + (lane - MI(agent_uadr)[ag]));
  }
#endif
  if (!COH && lane < mdl.nu) {   // fused rollout: the policy phase has put the step's actions into S(ctrl) itself
    const float PT_GAS* act0 = pt_global(a.actions) + (size_t)e * 2 * a.act_stride;
    int ag = lane >= MI(agent_uadr)[1] ? 1 : 0;
    S(ctrl)[lane] = (double)act0[ag * a.act_stride + (lane - MI(agent_uadr)[ag])];
  }
  SYNC();
  // torso xy before the step (agents.py:216-217) is parked in LDS so nothing but the context stays live across the
  // twenty forward-dynamics evaluations (keeps the kernel within the two-waves-per-SIMD register budget)
  if (lane < 2) { int qa = MI(agent_qposadr)[lane]; S(stash)[2 * lane] = S(qpos)[qa]; S(stash)[2 * lane + 1] = S(qpos)[qa + 1]; }
  SYNC();
  PROF(17);
  // bad-value guard, entry half: a state that already fails the test (host-imposed, or left by a launch that was cut short) is
  // not integrated at all; the exit half sits in the epilogue.  Checked per env step, not per mj_step: a flag that lives across
  // the twenty forward-dynamics evaluations costs the register budget more than stepping a lost state to the end (all loops
  // of the pipeline are bounded; NaN comparisons fall through)
  // (nothing stays live for it: a skipped state is still bad when the exit half looks)
  if (!state_is_bad(c)) mj_steps(c, mdl.frame_skip);
  PROF(18);
  int* cnt = a.counters + 4 * e;
  int num_steps = hand_load<COH>(cnt), reset_count = hand_load<COH>(cnt + 1);
  double* st = a.state + (size_t)e * a.state_stride;
  double ep_ret = hand_load<COH>(st + mdl.nq + 2 * mdl.nv), ep_dense = hand_load<COH>(st + mdl.nq + 2 * mdl.nv + 1);
  double before[2][2] = {{S(stash)[0], S(stash)[1]}, {S(stash)[2], S(stash)[3]}};
  // ---- game rules (sumo.py:120-202), evaluated redundantly by every lane (wave-uniform result)
  double after[2][2], z[2];
  for (int g = 0; g < 2; g++) {
    int qa = MI(agent_qposadr)[g];
    after[g][0] = S(qpos)[qa]; after[g][1] = S(qpos)[qa + 1]; z[g] = S(qpos)[qa + 2];
  }
  num_steps++;
  const double lim = mdl.tatami_size + 0.1;
  const double adjz = c.P->adjust_z;   // sumo.py:147,157 read get_qpos(): the lose test sees the adjusted z
  int lost[2];
  for (int g = 0; g < 2; g++) {
    double mx = fabs(after[g][0]) > fabs(after[g][1]) ? fabs(after[g][0]) : fabs(after[g][1]);
    lost[g] = (z[g] + adjz < 0.29) || (mx >= lim);
  }
  const double dt = MF(opt)[SUMO_OPT_TIMESTEP] * mdl.frame_skip;
  int dn = 0;
  double inf[2][SUMO_INFO_STRIDE];
#pragma unroll
  for (int g = 0; g < 2; g++) {
    int o = 1 - g, flags = 0;
    double ctrl_r = -0.1 * (double)sumsq_f32_ctrl(S(ctrl) + MI(agent_uadr)[g], MI(agent_nu)[g]);   // the actions as the step received them
    double lose = lost[g] ? -2000.0 : 0.0, win = lost[o] ? 2000.0 : 0.0;
    if (lost[g] || lost[o]) dn = 1;
    if (lost[o]) flags |= 1;
    double main_r = win + lose;
    if (num_steps > mdl.timestep_limit) { main_r += -1000.0; dn = 1; }
    double mv[2] = {(after[g][0] - before[g][0]) / dt, (after[g][1] - before[g][1]) / dt};
    double dir[2] = {after[o][0] - before[g][0], after[o][1] - before[g][1]};
    double nrm = sqrt(dir[0] * dir[0] + dir[1] * dir[1]);
    dir[0] /= nrm; dir[1] /= nrm;
    double proj = mv[0] * dir[0] + mv[1] * dir[1];
    double move = (proj > 0 ? proj : 0.0) * 0.1;
    double push = -10.0 * slow_exp(-sqrt(after[o][0] * after[o][0] + after[o][1] * after[o][1]));
    double shaping = ctrl_r + push + move;
    inf[g][0] = ctrl_r; inf[g][1] = lose; inf[g][2] = win; inf[g][3] = main_r; inf[g][4] = move; inf[g][5] = push;
    inf[g][6] = shaping; inf[g][7] = (double)flags;
  }
  // per-env divergence guard: a state that failed the bad-value test (during the stepping or after its last mj_step) ends the
  // episode with zero rewards and info flag 4; the auto-reset below replaces it, the engine counts it (sumo_stats[8])
  const int diverged = state_is_bad(c);
  c.st_diverged += diverged;
  if (diverged) {
#pragma unroll
    for (int g = 0; g < 2; g++) {
#pragma unroll
      for (int k = 0; k < SUMO_INFO_STRIDE; k++) inf[g][k] = 0.0;
      inf[g][7] = 4.0;
    }
    dn = 1;
  }
  ep_ret += inf[0][3] + inf[0][6];
  ep_dense += inf[0][6];
  if (!diverged && dn && inf[0][3] == -1000.0) { inf[0][7] += 2.0; inf[1][7] += 2.0; }
  if (lane == 0) {
    double* io = a.info + (size_t)e * 2 * SUMO_INFO_STRIDE;
#pragma unroll
    for (int g = 0; g < 2; g++)
#pragma unroll
      for (int k = 0; k < SUMO_INFO_STRIDE; k++) hand_store<COH>(io + g * SUMO_INFO_STRIDE + k, inf[g][k]);
    if (COH) {   // what the rollout's post phase needs of this step stays in LDS (nothing written in a launch is read back from HBM)
      double* sh = S(stash) + 5;
      sh[0] = inf[0][6]; sh[1] = inf[0][3]; sh[2] = inf[1][6]; sh[3] = inf[1][3]; sh[4] = dn ? ep_ret : 0.0;
      ((int*)(sh + 5))[0] = dn ? num_steps : 0; ((int*)(sh + 5))[1] = dn;
    }
  }
  // both agents' flags as one 16-bit store (one coherent store on the hand-over path)
  if (lane == 0) hand_store<COH>((uint16_t*)(a.done + 2 * e), (uint16_t)(dn ? 0x0101 : 0));
  if (lane == 0) { hand_store<COH>(a.ep_r + e, dn ? ep_ret : 0.0); hand_store<COH>(a.ep_dr + e, dn ? ep_dense : 0.0); hand_store<COH>(a.ep_l + e, dn ? num_steps : 0); }
  if (dn) {  // subproc_vec_env.py:13-16: auto-reset, reset observation replaces the terminal one
    reset_state(c, pt_global(a.seeds)[e], (uint32_t)reset_count);
    reset_count++;
    num_steps = 0; ep_ret = 0; ep_dense = 0;
  }
  write_obs<COH>(c, a.obs + (size_t)e * 2 * a.obs_stride, a.obs_stride, num_steps);
  const unsigned rec_out = store_state<COH>(c, a, e);
  if (COH && lane == 0) {   // sequence tag + checksum of the record just written (the next wave checks them first)
    const int k1 = ((const int*)(S(stash) + 4))[1] + 1;
    hand_store<true>(cnt + 3, (int)(rec_out + (unsigned)(k1 == 1 && a.dbg_fault_env == e)));   // dbg_fault_env: injected fault (tests)
    hand_store<true>(cnt + 2, a.seq_base + k1);
  }
  if (lane == 0) {
    hand_store<COH>(cnt, num_steps); hand_store<COH>(cnt + 1, reset_count);
    hand_store<COH>(st + mdl.nq + 2 * mdl.nv, ep_ret); hand_store<COH>(st + mdl.nq + 2 * mdl.nv + 1, ep_dense);
  }
  PROF(19);
  // work estimate for the next launch's longest-first schedule (sumo_step): Newton iterations dominate the variation
  // (a contention-independent proxy; sorting by the measured cycle count of the previous step schedules no better)
  // (least-squares fit of measured wave times, tools/slot_trace.py: Newton iterations, contacts, dense-path forwards)
  if (lane == 0 && a.cost) { const int w = 1000 + 12 * c.st_newton + 10 * c.st_ncon + 60 * c.st_dense; pt_global(a.cost)[e] = w < 65535 ? w : 65535; }
  if (a.trace && lane == 0) {
    a.trace[4 * e + 1] = wall_clock64();
    a.trace[4 * e + 2] = (unsigned long long)c.st_newton | ((unsigned long long)c.st_ncon << 32);
    a.trace[4 * e + 3] = (unsigned long long)c.st_dense | ((unsigned long long)c.st_cross << 16) | ((unsigned long long)c.st_nefc << 32);
  }
}

template <int SL> struct LayoutSel { typedef Layout type; };
template <> struct LayoutSel<1> { typedef LayoutAntAnt type; };
template <> struct LayoutSel<2> { typedef LayoutSpiderSpider type; };

template <int NV, int SL = 0>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(SUMO_WPE_OF(NV), SUMO_WPE_OF(NV)))) sumo_step_kernel(const Params* P, StepArgs a) {
  Ctx<NV, typename LayoutSel<SL>::type> c;
  ctx_init(c, P, smem_dyn);
  const int lane = c.lane;
  if ((int)blockIdx.x < a.rank_blocks) { sched_rank(a.rank_cost, a.N, a.rank_perm, blockIdx.x, lane); return; }
  const int bid = (int)blockIdx.x - a.rank_blocks;
  if (bid >= a.N) return;
  const int e = a.perm ? a.perm[bid] : bid;
  if (a.perm && bid < (a.N >> 3)) __builtin_amdgcn_s_setprio(1);   // predicted-longest eighth of the launch: issue ahead of the SIMD mate
#ifdef SUMO_DBG_POISON_LDS
  poison_lds(P, lane);
#endif
#ifdef SUMO_DBG_DUMP
#ifdef SUMO_DBG_DUMP_ALL   /* every env dumps: the buffer holds [N][20][8][64] doubles */
  c.dbg = a.dbg_qacc ? a.dbg_qacc + (size_t)e * (20 * 8 * 64) : nullptr;
#else
  c.dbg = e == 0 ? a.dbg_qacc : nullptr;
#endif
#endif
  env_step_body(c, a, e);
  flush_stats(c, a.stats);
}

// ---------------------------------------------------------------------------------------------------------
// cfrc_mode = rne_post: the contact-force entries of the observations as a MuJoCo 2.1 WITH force sensors
// would show them.  The reference's scenes have no such sensor, so its cfrc_ext is zero and `zero` is the default (and what
// sumo_step writes); this optional second launch fills the entries in afterwards and costs most of another env step: it
// repeats the first frame_skip - 1 sub-steps from the pre-step state (saved by the host before sumo_step) to reach the state
// the LAST mj_step started from -- mj_forward evaluates sensors, hence mj_rnePostConstraint, once per mj_step at its start
// state; the RK4 sub-stages skip them -- evaluates forward() there, turns the solution into the pyramid-row forces
// f = -D min(J qacc - aref, 0), recomputes the contact geometry (the records shared the mass matrix's storage) and sums,
// per body, -wrench (body 1) / +wrench (body 2) about the subtree CoM of the body's agent: [torque ; force], world axes.
// The hot kernels are untouched by this mode.  Envs whose episode ended in the step keep the zeros of their reset observation.
// ---------------------------------------------------------------------------------------------------------
struct CfrcArgs {
  const double* prev_state;   // [N][state_stride]: the state before the step
  double* fbuf;               // [N][5 * maxcon] scratch: row forces | friction coefficients
  double* cfrc_out;           // [N][nbody][6] or NULL (tests)
};

template <int NV>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(SUMO_WPE_OF(NV), SUMO_WPE_OF(NV))))
sumo_cfrc_kernel(const Params* P, StepArgs a, CfrcArgs q) {
  Ctx<NV> c;
  ctx_init(c, P, smem_dyn);
  const sumo_model_t& mdl = P->mdl;
  const int e = blockIdx.x, lane = c.lane, nb = mdl.nbody;
  if (e >= a.N) return;
  if (q.cfrc_out) for (int i = lane; i < 6 * nb; i += WAVE) q.cfrc_out[(size_t)e * 6 * nb + i] = 0.0;
  if (a.done[2 * e]) return;
  StepArgs ap = a;
  ap.state = const_cast<double*>(q.prev_state);
  load_state(c, ap, e);
  if (lane < mdl.nu) {
    const float PT_GAS* act0 = pt_global(a.actions) + (size_t)e * 2 * a.act_stride;
    const int ag = lane >= MI(agent_uadr)[1] ? 1 : 0;
    S(ctrl)[lane] = (double)act0[ag * a.act_stride + (lane - MI(agent_uadr)[ag])];
  }
  SYNC();
  if (state_is_bad(c)) return;
  if (mdl.frame_skip > 1) mj_steps(c, mdl.frame_skip - 1);
  c.use_prev = 0;
  forward(c);
  // pyramid-row forces of the solution (x = qacc): rows 4 ci + k of contact ci; limit rows carry no external force
  const int ncon = c.ncon, maxcon = c.L.maxcon;
  double* fb = q.fbuf + (size_t)e * 5 * maxcon;
  contact_Jx(c, S(x));
  for (int r = lane; r < 4 * ncon; r += WAVE) {
    const double jar = row_Jx(c, r) - S(aref)[r];
    fb[r] = jar < 0 ? -S(D)[r >> 2] * jar : 0.0;
  }
  for (int ci = lane; ci < ncon; ci += WAVE) fb[4 * maxcon + ci] = S(cpar)[ci];
  __threadfence();
  SYNC();
  // contact points / frames / bodies again (same state, same order), subtree CoMs
  position_velocity(c);
  collision(c);
  const int nc2 = c.ncon < ncon ? c.ncon : ncon;   // (make_constraint may have cut the list to the Jacobian pool)
  KCONSTS();
  double w[6] = {0, 0, 0, 0, 0, 0};
  const int b = lane, ag = role_agent(c);   // one body per lane: build_aux refuses scenes with nbody > WAVE at sumo_create ("scene too large for one wavefront per env")
  if (b > 0 && b < nb) {
    const double* com = S(com) + 3 * ag;
    for (int ci = 0; ci < nc2; ci++) {
      const int* cb = c.si + c.L.con_b + 4 * ci;
      const int side = cb[1] == b ? 1 : (cb[0] == b ? 0 : -1);
      if (side < 0) continue;
      const double* cd = S(cond) + 14 * ci;
      const double f0 = fb[4 * ci], f1 = fb[4 * ci + 1], f2 = fb[4 * ci + 2], f3 = fb[4 * ci + 3], mu = fb[4 * maxcon + ci];
      const double fc[3] = {(f0 + f1) + (f2 + f3), mu * (f0 - f1), mu * (f2 - f3)};
      double F[3], arm[3], tq[3];
#pragma unroll
      for (int k = 0; k < 3; k++) { F[k] = cd[4 + k] * fc[0] + cd[7 + k] * fc[1] + cd[10 + k] * fc[2]; arm[k] = cd[1 + k] - com[k]; }
      cross3(tq, arm, F);
      const double sg = side ? 1.0 : -1.0;
#pragma unroll
      for (int k = 0; k < 3; k++) { w[k] += sg * tq[k]; w[3 + k] += sg * F[k]; }
    }
    if (q.cfrc_out)
      for (int k = 0; k < 6; k++) q.cfrc_out[((size_t)e * nb + b) * 6 + k] = w[k];
    // agents.py:192-208: |clip(cfrc_ext, +-100)| of the own bodies, then (for the other side) of this agent's torso
    const int i0 = MI(agent_bodyadr)[ag], o = 1 - ag;
    float* ob = a.obs + (size_t)e * 2 * a.obs_stride;
    float* own = ob + ag * a.obs_stride + MI(agent_nq)[ag] + MI(agent_nv)[ag] + 6 * (b - i0);
#pragma unroll
    for (int k = 0; k < 6; k++) own[k] = (float)fabs(fmin(fmax(w[k], -100.0), 100.0));
    if (b == i0) {
      float* opp = ob + o * a.obs_stride + MI(agent_nq)[o] + MI(agent_nv)[o] + 6 * MI(agent_nbody)[o] + 7;
#pragma unroll
      for (int k = 0; k < 6; k++) opp[k] = (float)fabs(fmin(fmax(w[k], -100.0), 100.0));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Fused rollout: K consecutive self-play rollout steps of an env in ONE launch (reference runner.py:62-151 for MLP(64,64)
// policies).  The wave that owns env e evaluates the five policy / value passes of a step itself -- the env's two
// observations are rows 0 and 1 of an MFMA tile, the three trunks (learner policy, opponent policy, learner value) run through
// the same device functions as the batched PPO kernels, so every number equals the stepwise path bit for bit -- records
// obs / actions / values / neglogps / done flags straight into the [agent][time][env] rollout buffers, steps its env and
// records the mixed reward and the episode statistics.  No launch boundary, no policy launch and no per-step barrier over
// the envs remain between two env steps; each env may face its own frozen opponent snapshot (opp_idx).
// ---------------------------------------------------------------------------------------------------------
#ifdef SUMO_POLICY_PROBE   /* development build: the per-env phase clock also splits the MLP policy phase (tools/fused_probe.py --probe) */
#define PROF_STRIDE 12
#define PPROBE(slot) do { if (r.prof && lane == 0) { const unsigned long long t_ = wall_clock64(); atomicAdd(r.prof + PROF_STRIDE * e + (slot), t_ - tp_); tp_ = t_; } } while (0)
#else
#define PROF_STRIDE 4
#define PPROBE(slot) do { } while (0)
#endif
// The policy-zoo tables of a launch (POLICY 4 .. 12), one struct per family.  Every zoo mode reads its table(s) from the two members
// RolloutArgs::zm / zl, which no other mode reads; a league (POLICY 11 / 12) fills both, and RolloutArgs::tile_net then holds the
// entry of every 16-env tile of the whole env set: [0, zm.n) = that row of the MLP table, [zm.n, zm.n + zl.n) = row entry - zm.n of
// the LSTM table.
struct ZooMlpTable {
  const float* params;               // [n][L.P]
  const float* filt;                 // [n][2][D]: mean | 1 / std
  float clip;
  int n, D;                          // entries, input width (the first D columns of the scene's observation)
  ParamLayout L;                     // make_layout(D, A)
};
// A zoo LSTM net's parameter row follows the order of sumo_zoo_lstm.  Its cell's rows (embedding [64] | previous latent [64] | new
// latent [64], 16-byte aligned) start sc_off floats from the scratch base (lds_off); agent 1's recurrent state [N][128] (c | h)
// travels in RolloutArgs::st1.
struct ZooLstmTable {
  const float* params;               // [n][P]
  const float* filt;                 // [n][2][D]: mean | 1 / std
  float clip, forget_bias;
  int n, D, A, P;
  int sc_off;
  int emb;                           // embedding width (the table's emb_dim, 64).  Deliberately a launch field and not a literal:
                                     // lstm_gates_valu's chunk loop runs (emb + 64) / 4 trips, and it keeps its ring of four
                                     // chunk buffers only while that count is a run-time value, as it is for the LSTM(128)
                                     // nets (their D is a launch field too).  The loop is shared with modes 1 and 3, so it
                                     // carries no unroll pragma of its own.
};
// One side of the co-training launch (POLICY 16): agent g of a match-up whose two sides may differ in observation and action width
// acts with row tile_row[tile] of its own table of MLP(64,64) rows and keeps its own record [T][Ntot][...] (noise: RolloutArgs::noise0 / 1).
struct PairSideArgs {
  const float* table;                // [nrows][row_stride], a row in ppo_forward's flat order
  const int32_t* tile_row;           // [Ntot / 16]: the row of every 16-env tile of the whole env set, or NULL (row 0)
  float *obs, *act, *val, *nlp;      // written on the side's recording tiles only
  uint8_t* done;
  int nrows, row_stride;
  int record_row;                    // the side records (and evaluates its value net) on the tiles that play this row; < 0: on every tile
  ParamLayout L;                     // make_layout(D_g, A_g)
};
struct RolloutArgs {
  const float *learner, *opponent;   // flat parameter vectors; opponent: the self-play snapshot pool [npool][P]
  const int32_t* opp_idx;            // [N] snapshot (zoo modes: table row) per env or NULL
  const float *noise0, *noise1;      // [T][N][A]
  float *obs, *act, *rew, *val, *nlp, *onlp;   // the rollout record [2][T][Ntot][...] (the match modes write none)
  uint8_t *done, *ep_done;           // [2][T][Ntot], [T][Ntot]
  double* ep_r;                      // [T][Ntot]
  int32_t* ep_l;                     // [T][Ntot]
  double alpha;
  int T, Ntot, env_offset, s0, K, XS, lds_off;   // lds_off: LDS offset (doubles) of the policy scratch (the mass-matrix region)
  int* sched;                        // ticket counter | abort flag | finished steps per env [N] (zeroed by the host per launch)
  unsigned long long* prof;          // development (sumo_debug_trace): [N][4] wave start, end, ticks in the policy phases, ticks in the env steps (100 MHz)
  ParamLayout L;                     // the MLP learner's / checkpoints' layout
  // recurrent policies (sumo_rollout_steps_lstm): the learner's net (matches: the prototype), the opponent snapshots (device array)
  // with the snapshot of every 16-env tile of the whole env set (NULL: snapshot 0; zoo modes: the table row / league entry of the
  // tile), and the acting nets' states [N][2 hidden] (c | h) per agent
  ppo_lstm_net lnet;
  const ppo_lstm_net* onets;
  const int32_t* tile_net;
  float *st0, *st1;
  // checkpoint-vs-checkpoint matches (sumo_match_steps, POLICY 2): agent 0 acts with snapshot idx0[e], agent 1 with idx1[e] of
  // snaps [nsnap][P]; noise0 / noise1 NULL = deterministic play.  score [N][3] = {agent-0 wins, agent-1 wins, draws} of the env,
  // counted while their sum is below quota.  An env's counters cross waves between its tickets like its record: lane 0 of the
  // owning wave reads them with hand_load<true> and writes them with hand_store<true> before the s_waitcnt vmcnt(0) that precedes
  // the progress store, so the next owner (which polls prog[e] first) sees them.
  const float* snaps;
  const int32_t *idx0, *idx1;
  int* score;
  int nsnap, quota;
  // policy-zoo opponents (POLICY 4 .. 12); appended, so every field above keeps the offset the modes 0 .. 3 read it at
  ZooMlpTable zm;
  ZooLstmTable zl;
  // cross-family matches (POLICY 13): the agent the LSTM(128) checkpoints play (the other one plays the MLP(64,64) checkpoints) and
  // the size of their table onets (nsnap is the size of snaps); appended like the zoo tables
  int lstm_side, nsnap_lstm;
  // opponent-data reuse for a recurrent learner (POLICY 15): the learner's shadow state along agent 1's stream [N][2 hidden]; appended
  float* st2;
  // co-training on a match-up of two species (POLICY 16): the two sides; appended.  It reuses noise0 / noise1 (here [T][Ntot][A_g], the
  // columns of the whole env set), rew, ep_*, T .. K, alpha, XS (one row stride for both x rows) and lds_off
  PairSideArgs pair[2];
};

// ---- pieces shared by the four policy phases (each reads a / r through the references its phase received) ----
// The env's two observations through the hand-over loads into rows 0 / 1 of the LDS tile x [2][XS].  PAD: columns D .. XS are
// zero-filled; REC: the observations also go into the rollout record (runner.py:98-101).
template <bool PAD, bool REC, class SA, class RA>
__device__ __forceinline__ void policy_load_obs(const SA& a, const RA& r, int e, int lane, float* x, int D, int XS, size_t slot0 = 0, size_t slot1 = 0) {
  const float* ob = a.obs + (size_t)e * 2 * a.obs_stride;
  for (int k = lane; k < (PAD ? XS : D); k += WAVE) {
    float o0 = 0.0f, o1 = 0.0f;
    if (!PAD || k < D) {
      o0 = hand_load<true>(ob + k); o1 = hand_load<true>(ob + a.obs_stride + k);
      if (REC && PAD) { pt_global(r.obs)[slot0 * D + k] = o0; pt_global(r.obs)[slot1 * D + k] = o1; }   // (one predicated region)
    }
    x[k] = o0; x[XS + k] = o1;
    if (REC && !PAD) { pt_global(r.obs)[slot0 * D + k] = o0; pt_global(r.obs)[slot1 * D + k] = o1; }
  }
}

// Done flags of the previous step (agent 0 in the low byte, agent 1 in the next): the masks M of the recurrent nets; lanes 0 / 1
// append agent 0's / agent 1's flag to the rollout record.
template <class SA>
__device__ __forceinline__ unsigned policy_prev_done(const SA& a, int e) { return hand_load<true>((const uint16_t*)(a.done + 2 * e)); }
template <class RA>
__device__ __forceinline__ void policy_record_done(const RA& r, int lane, size_t slot0, size_t slot1, unsigned dn) {
  pt_global(r.done)[lane == 0 ? slot0 : slot1] = (uint8_t)(dn >> (8 * lane));
}

// Snapshot rows of env e's two sides (matches).  An index outside [0, nsnap) raises the launch's abort flag and plays row 0.
template <class SA, class RA>
__device__ __forceinline__ void policy_snapshot_rows(const SA& a, const RA& r, int e, int lane, int& j0, int& j1) {
  j0 = pt_global(r.idx0)[e]; j1 = pt_global(r.idx1)[e];
  if ((unsigned)j0 >= (unsigned)r.nsnap || (unsigned)j1 >= (unsigned)r.nsnap) {
    if (lane == 0) __hip_atomic_store(pt_global(a.abort_flag), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    j0 = (unsigned)j0 < (unsigned)r.nsnap ? j0 : 0; j1 = (unsigned)j1 < (unsigned)r.nsnap ? j1 : 0;
  }
}

// Column i of both actions (lanes i < A): REC into the rollout record; into the env's action buffer (output only, read back by
// the next owner of the env) and into the step's control vector.
template <bool REC, class C, class SA, class RA>
__device__ __forceinline__ void policy_commit_actions(C& c, const SA& a, const RA& r, int e, int i, float act0, float act1, int A = 0, size_t slot0 = 0, size_t slot1 = 0) {
  if (REC) { pt_global(r.act)[slot0 * A + i] = act0; pt_global(r.act)[slot1 * A + i] = act1; }
  float* ae = const_cast<float*>(a.actions) + (size_t)e * 2 * a.act_stride;
  hand_store<true>(ae + i, act0); hand_store<true>(ae + a.act_stride + i, act1);
  const auto& mdl = model_view(c);
  S(ctrl)[MI(agent_uadr)[0] + i] = (double)act0; S(ctrl)[MI(agent_uadr)[1] + i] = (double)act1;
}

// Index of column i of env e's draw at step s in noise0 / noise1 [T][N][A]
template <class SA>
__device__ __forceinline__ size_t policy_noise_index(const SA& a, int e, int s, int A, int i) { return ((size_t)s * a.N + e) * A + i; }

// The step's scalars of the rollout record (lane 0): the learner's / the opponent's neglogp of both actions, the learner's values
template <class RA>
__device__ __forceinline__ void policy_record_scalars(const RA& r, size_t slot0, size_t slot1, float nlp0, float nlp1, float onlp0, float onlp1, float v0, float v1) {
  pt_global(r.nlp)[slot0] = nlp0; pt_global(r.nlp)[slot1] = nlp1; pt_global(r.onlp)[slot0] = onlp0; pt_global(r.onlp)[slot1] = onlp1;
  pt_global(r.val)[slot0] = v0; pt_global(r.val)[slot1] = v1;
}

// Recurrent state rows [2 NH] (c | h) cross waves like the env's record.  A lane owns the units j0 = 2 lane and j0 + 1:
// lstm_state_pair loads their entries at p (one 8-byte hand-over load) masked by `keep` into out[0..1] (registers or LDS),
// lstm_bias_pair prefetches their four gate biases, lstm_state_store writes unit j's new (c, h) back.
__device__ __forceinline__ void lstm_state_pair(const float* p, float keep, float* out) {
  union { unsigned long long u; float f[2]; } q;
  q.u = hand_load<true>((const unsigned long long*)p); out[0] = q.f[0] * keep; out[1] = q.f[1] * keep;
}
template <int NH>
__device__ __forceinline__ void lstm_bias_pair(const float PT_GAS* b, int j0, float (&bz)[4][2]) {
#pragma unroll
  for (int g = 0; g < 4; g++) { bz[g][0] = b[g * NH + j0]; bz[g][1] = b[g * NH + j0 + 1]; }
}
template <int NH>
__device__ __forceinline__ void lstm_state_store(float* sp, int j, const LstmCell& cell) {
  hand_store<true>(sp + j, cell.cn); hand_store<true>(sp + NH + j, cell.hn);
}

// MLP policy phase (POLICY 0).  The three trunks of a step -- learner policy, opponent policy (snapshot opp_idx[e]), learner value --
// run in ONE pass on the vector ALU (ppo_tile.h mlp_rows_valu<3, 2>: lane j owns hidden unit j of all three nets, one ring of weight
// rows through both layers), in the accumulation order of the MFMA tiles of ppo_selfplay_kernel, so every number equals the
// step-by-step path bit for bit.  LDS (floats, from lds_off; place_mlp_scratch(valu_nets = 3)): x [2][XS], zero in columns
// D .. XS | activation rows [3][2][PT_VS].
template <class C, class SA, class RA>
__device__ __forceinline__ void rollout_policy_phase(C& c, const SA& a, const RA& r, int e, int s) {
  const int lane = c.lane, i = lane & 15, kq = lane >> 4;
  const int D = r.L.D, A = r.L.A, XS = r.XS;
  float* xbuf = (float*)(c.sm + r.lds_off);
  float* hb = xbuf + 2 * XS;
  const size_t col = (size_t)r.env_offset + e;
  const size_t slot0 = ((size_t)0 * r.T + s) * r.Ntot + col, slot1 = ((size_t)1 * r.T + s) * r.Ntot + col;
#ifdef SUMO_POLICY_PROBE
  unsigned long long tp_ = wall_clock64();
#endif
  const int oiv = r.opp_idx ? pt_global(r.opp_idx)[e] : 0;   // (in flight during the observation loads)
  policy_load_obs<true, true>(a, r, e, lane, xbuf, D, XS, slot0, slot1);
  if (lane < 2) policy_record_done(r, lane, slot0, slot1, policy_prev_done(a, e));
  const float PT_GAS* lp = pt_global(r.learner);
  const float PT_GAS* op = pt_global(r.opponent) + (size_t)__builtin_amdgcn_readfirstlane(oiv) * r.L.P;
  // what the heads need is requested with the first weight rows, not behind the trunks
  const bool colk = i < A;
  const float lsL = colk ? lp[r.L.logstd + i] : 0.0f, lsO = colk ? op[r.L.logstd + i] : 0.0f;
  const bool ok = colk && kq == 0;                  // rows 0 and 1 of a head live in the first 16 lanes
  const size_t nz = policy_noise_index(a, e, s, A, i);
  const float n0 = ok ? pt_global(r.noise0)[nz] : 0.0f, n1 = ok ? pt_global(r.noise1)[nz] : 0.0f;
  wave_sync();
  PPROBE(4);
  const Net nets[3] = {pi_net((const float*)lp, r.L), pi_net((const float*)op, r.L), vf_net((const float*)lp, r.L)};
  float m[3][2];                                    // [learner mean | opponent mean | learner value][row]
  mlp_rows_valu<3, 2>(nets, xbuf, XS, D, hb, lane, m);
  PPROBE(7);
  // heads: row 0 = agent 0 (learner acts, opponent scores), row 1 = agent 1 (opponent acts, learner scores and values)
  const float stdL = expf(lsL), stdO = expf(lsO);
  const float sumL = row16_sum(lsL), sumO = row16_sum(lsO);
  float act0 = 0.0f, act1 = 0.0f;
  const float nlp0 = gauss_row(m[0][0], stdL, sumL, ok, true, n0, act0, A);      // learner samples for agent 0 ...
  const float onlp0 = gauss_row(m[1][0], stdO, sumO, ok, false, 0.0f, act0, A);  // ... the opponent net scores that action
  const float onlp1 = gauss_row(m[1][1], stdO, sumO, ok, true, n1, act1, A);     // opponent samples for agent 1 ...
  const float nlp1 = gauss_row(m[0][1], stdL, sumL, ok, false, 0.0f, act1, A);   // ... the learner scores it
  if (ok) policy_commit_actions<true>(c, a, r, e, i, act0, act1, A, slot0, slot1);
  if (lane == 0) policy_record_scalars(r, slot0, slot1, nlp0, nlp1, onlp0, onlp1, m[2][0], m[2][1]);
  PPROBE(8);
  wave_sync();   // the action buffer is read back by the env step (other lanes), the scratch region becomes the mass matrix again
}

// The same phase for recurrent policies (baselines lstm(128) with shared value head; Runner._step_group's recurrent branch,
// reference runner.py:62-96 with the S / M feeds of models.py:163-170).  Five evaluations per step, two passes over weights:
//   opponent net: row A = (obs 1, agent 1's state)  -> action 1, its neglogp (opponent_neglogp), agent 1's NEW state
//                 row B = (obs 0, zero state)        -> the opponent's likelihood of action 0 (runner.py:85 feeds no state)
//   learner net:  row C = (obs 0, agent 0's state)  -> action 0, neglogp, value, agent 0's new state
//                 row D = (obs 1, agent 1's new state, masked again) -> the value recorded for agent 1 (runner.py:93)
//                 row E = (obs 1, zero state)        -> the learner's likelihood of action 1
// Gate pre-activations run on the vector ALU in the MFMA tiles' accumulation order (lstm_gates_valu), cell update and heads
// through the functions ppo_lstm_step_kernel uses: every number equals the launch-per-evaluation path bit for bit.
// LDS (floats, from lds_off): x [2][XS] | zero row [NH] | previous latents [3][NH] | new latents [3][NH].
//
// REUSE (POLICY 15, sumo_rollout_steps_lstm_reuse: opponent-data reuse for a recurrent learner).  The opponent's pass is the one
// above; the learner's pass has TWO rows, and rows D and E give way to
//                 row D' = (obs 1, the learner's SHADOW state along agent 1's stream r.st2, masked by agent 1's done flag)
//                          -> the value AND the neglogp of action 1 recorded for agent 1, the new shadow state
// -- what BPTT re-evaluates along agent 1's sequence, so the recorded "old" numbers belong to the function that is trained.  The
// shadow state crosses waves like the other two.  Same LDS region (one new latent row stays unused).
template <int NH, bool REUSE = false, class C, class SA, class RA>
__device__ __forceinline__ void rollout_policy_phase_lstm(C& c, const SA& a, const RA& r, int e, int s) {
  const int lane = c.lane;
  const auto& NL = r.lnet;
  const int D = NL.ob_dim, A = NL.ac_dim, XS = r.XS;
  float* xo = (float*)(c.sm + r.lds_off);
  float* hz = xo + 2 * XS;
  float* hp = hz + NH;
  float* hn = hp + 3 * NH;
  const size_t col = (size_t)r.env_offset + e;
  const size_t slot0 = ((size_t)0 * r.T + s) * r.Ntot + col, slot1 = ((size_t)1 * r.T + s) * r.Ntot + col;
  policy_load_obs<true, true>(a, r, e, lane, xo, D, XS, slot0, slot1);
  const unsigned dn = policy_prev_done(a, e);
  if (lane < 2) policy_record_done(r, lane, slot0, slot1, dn);
  const float keep0 = 1.0f - (float)(dn & 0xff), keep1 = 1.0f - (float)((dn >> 8) & 0xff);
  // the acting nets' states: lane owns the units 2 lane, 2 lane + 1
  float* s0p = r.st0 + (size_t)e * 2 * NH;
  float* s1p = r.st1 + (size_t)e * 2 * NH;
  const int j0 = 2 * lane;
  float c0[2], c1[2], cD[2];
  lstm_state_pair(s0p + j0, keep0, c0);
  lstm_state_pair(s1p + j0, keep1, c1);
  lstm_state_pair(s0p + NH + j0, keep0, hp + NH + j0);
  lstm_state_pair(s1p + NH + j0, keep1, hp + j0);
  float* s2p = nullptr;
  if constexpr (REUSE) {
    s2p = r.st2 + (size_t)e * 2 * NH;
    lstm_state_pair(s2p + j0, keep1, cD);
    lstm_state_pair(s2p + NH + j0, keep1, hp + 2 * NH + j0);
  }
  hz[j0] = 0.0f; hz[j0 + 1] = 0.0f;
  wave_sync();
  const ppo_lstm_net PT_GAS* NOp = pt_global(r.onets) + (r.tile_net ? pt_global(r.tile_net)[col >> 4] : 0);
  const bool ok = lane < A;
  const size_t nz = policy_noise_index(a, e, s, A, lane);
  float act0 = 0.0f, act1 = 0.0f, onlp1, mOB, stdO, sumO;
  {  // ---- opponent net: rows A, B
    const float *owx = NOp->wx, *owh = NOp->wh;
    const float PT_GAS* ob_ = pt_global(NOp->b);
    const float fb = NOp->forget_bias;
    float z[4][2][2], bz[4][2];
    lstm_bias_pair<NH>(ob_, j0, bz);   // (in flight during the gate sums)
    const float* const xr[2] = {xo + XS, xo};
    const float* const hr[2] = {hp, hz};
    lstm_gates_valu<NH, 2>(owx, owh, D, xr, hr, lane, z);
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int j = j0 + u;
      const float bi = bz[0][u], bf = bz[1][u] + fb, bo = bz[2][u], bu = bz[3][u];   // gate order i, f, o, u
      const LstmCell ca = lstm_cell(z[0][u][0], z[1][u][0], z[2][u][0], z[3][u][0], bi, bf, bo, bu, c1[u]);
      const LstmCell cb = lstm_cell(z[0][u][1], z[1][u][1], z[2][u][1], z[3][u][1], bi, bf, bo, bu, hz[j]);
      lstm_state_store<NH>(s1p, j, ca);                                              // agent 1's state after the opponent's step
      hn[j] = ca.hn; hn[NH + j] = cb.hn;
      if constexpr (!REUSE) { cD[u] = ca.cn * keep1; hp[2 * NH + j] = ca.hn * keep1; }   // row D: masked once more by the same flag
    }
    wave_sync();
    float m[2];
    lstm_heads_valu<NH, 2>(NOp->head_w, NOp->vf_w, A, hn, lane, m);
    const float hb = ok ? pt_global(NOp->head_b)[lane] : 0.0f, ls = ok ? pt_global(NOp->logstd)[lane] : 0.0f;
    stdO = expf(ls); sumO = row16_sum(ls);
    mOB = m[1] + hb;
    const float n1 = ok ? pt_global(r.noise1)[nz] : 0.0f;
    onlp1 = gauss_row(m[0] + hb, stdO, sumO, ok, true, n1, act1, A);     // the opponent samples for agent 1
    wave_sync();   // the latent rows are rewritten by the learner's pass
  }
  float nlp0, nlp1, onlp0, v0, v1;
  if constexpr (REUSE) {  // ---- learner net: rows C, D'
    // A two-row learner pass like lstm_learner_front's (POLICY 9, 10, 12), with row 2's (c, h) from the shadow state and one more
    // state store.  It is written out here and not drawn from a helper shared with that function and the branch below: a helper
    // would rewrite the source of modes 1, 9, 10 and 12, whose static-layout code objects this change keeps the parent's line for
    // line (DESIGN.md sections 18, 19), and whether they survive that has not been tried.  The pieces inside (lstm_bias_pair,
    // lstm_gates_valu, lstm_cell, lstm_state_store, lstm_heads_valu, gauss_row) exist once.
    const float fb = NL.forget_bias;
    float z[4][2][2], bz[4][2];
    lstm_bias_pair<NH>(pt_global(NL.b), j0, bz);
    const float* const xr[2] = {xo, xo + XS};
    const float* const hr[2] = {hp + NH, hp + 2 * NH};
    lstm_gates_valu<NH, 2>(NL.wx, NL.wh, D, xr, hr, lane, z);
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int j = j0 + u;
      const float bi = bz[0][u], bf = bz[1][u] + fb, bo = bz[2][u], bu = bz[3][u];
      const LstmCell cc = lstm_cell(z[0][u][0], z[1][u][0], z[2][u][0], z[3][u][0], bi, bf, bo, bu, c0[u]);
      const LstmCell cd = lstm_cell(z[0][u][1], z[1][u][1], z[2][u][1], z[3][u][1], bi, bf, bo, bu, cD[u]);
      lstm_state_store<NH>(s0p, j, cc);                                              // agent 0's state after the learner's step
      lstm_state_store<NH>(s2p, j, cd);                                              // the shadow state after agent 1's row
      hn[j] = cc.hn; hn[NH + j] = cd.hn;
    }
    wave_sync();
    float m[2];
    lstm_heads_valu<NH, 2>(NL.head_w, NL.vf_w, A, hn, lane, m);
    const float hb = ok ? pt_global(NL.head_b)[lane] : 0.0f, ls = ok ? pt_global(NL.logstd)[lane] : 0.0f;
    const float stdL = expf(ls), sumL = row16_sum(ls);
    const float vb = pt_global(NL.vf_b)[0];
    v0 = __shfl(m[0], 16) + vb; v1 = __shfl(m[1], 16) + vb;
    const float n0 = ok ? pt_global(r.noise0)[nz] : 0.0f;
    nlp0 = gauss_row(m[0] + hb, stdL, sumL, ok, true, n0, act0, A);      // the learner samples for agent 0 ...
    onlp0 = gauss_row(mOB, stdO, sumO, ok, false, 0.0f, act0, A);        // ... the opponent net (zero state) scores that action
    nlp1 = gauss_row(m[1] + hb, stdL, sumL, ok, false, 0.0f, act1, A);   // the learner (shadow state) scores the opponent's action
  } else {  // ---- learner net: rows C, D, E
    const float fb = NL.forget_bias;
    float z[4][2][3], bz[4][2];
    lstm_bias_pair<NH>(pt_global(NL.b), j0, bz);
    const float* const xr[3] = {xo, xo + XS, xo + XS};
    const float* const hr[3] = {hp + NH, hp + 2 * NH, hz};
    lstm_gates_valu<NH, 3>(NL.wx, NL.wh, D, xr, hr, lane, z);
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int j = j0 + u;
      const float bi = bz[0][u], bf = bz[1][u] + fb, bo = bz[2][u], bu = bz[3][u];
      const LstmCell cc = lstm_cell(z[0][u][0], z[1][u][0], z[2][u][0], z[3][u][0], bi, bf, bo, bu, c0[u]);
      const LstmCell cd = lstm_cell(z[0][u][1], z[1][u][1], z[2][u][1], z[3][u][1], bi, bf, bo, bu, cD[u]);
      const LstmCell ce = lstm_cell(z[0][u][2], z[1][u][2], z[2][u][2], z[3][u][2], bi, bf, bo, bu, hz[j]);
      lstm_state_store<NH>(s0p, j, cc);                                              // agent 0's state after the learner's step
      hn[j] = cc.hn; hn[NH + j] = cd.hn; hn[2 * NH + j] = ce.hn;
    }
    wave_sync();
    float m[3];
    lstm_heads_valu<NH, 3>(NL.head_w, NL.vf_w, A, hn, lane, m);
    const float hb = ok ? pt_global(NL.head_b)[lane] : 0.0f, ls = ok ? pt_global(NL.logstd)[lane] : 0.0f;
    const float stdL = expf(ls), sumL = row16_sum(ls);
    const float vb = pt_global(NL.vf_b)[0];
    v0 = __shfl(m[0], 16) + vb; v1 = __shfl(m[1], 16) + vb;
    const float n0 = ok ? pt_global(r.noise0)[nz] : 0.0f;
    nlp0 = gauss_row(m[0] + hb, stdL, sumL, ok, true, n0, act0, A);      // the learner samples for agent 0 ...
    onlp0 = gauss_row(mOB, stdO, sumO, ok, false, 0.0f, act0, A);        // ... the opponent net (zero state) scores that action
    nlp1 = gauss_row(m[2] + hb, stdL, sumL, ok, false, 0.0f, act1, A);   // the learner (zero state) scores the opponent's action
  }
  if (ok) policy_commit_actions<true>(c, a, r, e, lane, act0, act1, A, slot0, slot1);
  if (lane == 0) policy_record_scalars(r, slot0, slot1, nlp0, nlp1, onlp0, onlp1, v0, v1);
  wave_sync();
}

// Match policy phase (sumo_match_steps): two policy trunks, snapshot idx0[e] on the tile (its row 0 = agent 0's observation acts)
// and snapshot idx1[e] (its row 1 = agent 1's observation acts); no value net, no cross-scoring, nothing recorded.  The action is
// the mean (noise NULL, PPOModel.step(deterministic=True)) or mean + exp(logstd) * noise through gauss_row as ppo_forward samples.
// A snapshot index outside [0, nsnap) raises the launch's abort flag (sumo_rollout_status fails) and plays snapshot 0 instead.
template <class C, class SA, class RA>
__device__ __forceinline__ void rollout_policy_phase_match(C& c, const SA& a, const RA& r, int e, int s) {
  const int lane = c.lane, i = lane & 15, kq = lane >> 4;
  const int D = r.L.D, A = r.L.A, XS = r.XS;
  float* xbuf = (float*)(c.sm + r.lds_off);        // x [2][XS], zero in columns D .. XS | activation rows [2][2][PT_VS]
  float* hb = xbuf + 2 * XS;
  int j0, j1;
  policy_snapshot_rows(a, r, e, lane, j0, j1);
  policy_load_obs<true, false>(a, r, e, lane, xbuf, D, XS);
  const float PT_GAS* p0 = pt_global(r.snaps) + (size_t)__builtin_amdgcn_readfirstlane(j0) * r.L.P;
  const float PT_GAS* p1 = pt_global(r.snaps) + (size_t)__builtin_amdgcn_readfirstlane(j1) * r.L.P;
  const bool ok = i < A && kq == 0;                 // rows 0 and 1 of a head live in the first 16 lanes
  float ls0 = 0.0f, ls1 = 0.0f, n0 = 0.0f, n1 = 0.0f;
  if (r.noise0) {   // (requested with the first weight rows)
    ls0 = ok ? p0[r.L.logstd + i] : 0.0f; ls1 = ok ? p1[r.L.logstd + i] : 0.0f;
    const size_t nz = policy_noise_index(a, e, s, A, i);
    n0 = ok ? pt_global(r.noise0)[nz] : 0.0f; n1 = ok ? pt_global(r.noise1)[nz] : 0.0f;
  }
  wave_sync();
  const Net nets[2] = {pi_net((const float*)p0, r.L), pi_net((const float*)p1, r.L)};
  float m[2][2];                                    // both trunks in one pass on the vector ALU (mlp_rows_valu), as rollout_policy_phase
  mlp_rows_valu<2, 2>(nets, xbuf, XS, D, hb, lane, m);
  float act0 = m[0][0], act1 = m[1][1];
  if (r.noise0) {
    (void)gauss_row(m[0][0], expf(ls0), 0.0f, ok, true, n0, act0, A);
    (void)gauss_row(m[1][1], expf(ls1), 0.0f, ok, true, n1, act1, A);
  }
  if (ok) policy_commit_actions<false>(c, a, r, e, i, act0, act1);
  wave_sync();   // the action buffer is read back by the env step (other lanes), the scratch region becomes the mass matrix again
}

// ---- pieces of the match modes 3, 5, 6, 7, 13, 14 and of the zoo rollouts 4, 8 .. 12 (each exists once; the phases below compose them) ----
// Row j of a table of n entries, checked: an index outside [0, n) raises the launch's abort flag and plays row 0.
template <class SA>
__device__ __forceinline__ int policy_checked_row(const SA& a, int lane, int j, int n) {
  if ((unsigned)j >= (unsigned)n) {
    if (lane == 0) __hip_atomic_store(pt_global(a.abort_flag), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    j = 0;
  }
  return j;
}

// One side of an LSTM(128) match: agent g in {0, 1} acts with net jn of the device table onets on (obs g, its own state st_g[e] masked
// by the previous step's done flag) -- LstmPPOModel.step on one row, the S / M feeds of models.py:163-170.  Gate sums on the vector
// ALU in the MFMA tiles' order (lstm_gates_valu), cell update and Gaussian head through the functions ppo_lstm_step_kernel uses, so
// every number equals that kernel bit for bit.  No value head; the new state crosses waves like the LSTM rollout's.  xo: x [2][XS],
// zero-padded; hp / hn: previous / new latent [NH], free for the next side when the function returns.  act: the action's column in
// lanes < A -- by reference, not returned: returned, mode 3 on the 28-DoF dynamic layout spills three more vector registers.
template <int NH, class SA, class RA>
__device__ __forceinline__ void match_lstm_side(const SA& a, const RA& r, int e, int s, int lane, int g, int jn, unsigned dn, float* xo,
                                                float* hp, float* hn, float& act) {
  const int D = r.lnet.ob_dim, A = r.lnet.ac_dim;
  const bool ok = lane < A;
  const int j0 = 2 * lane;                           // lane owns the units 2 lane, 2 lane + 1
  const ppo_lstm_net PT_GAS* NT = pt_global(r.onets) + jn;
  const float keep = 1.0f - (float)((dn >> (8 * g)) & 0xff);
  float* sp = (g ? r.st1 : r.st0) + (size_t)e * 2 * NH;
  float cp[2];
  lstm_state_pair(sp + j0, keep, cp);
  lstm_state_pair(sp + NH + j0, keep, hp + j0);
  const float PT_GAS* b_ = pt_global(NT->b);
  const float fb = NT->forget_bias;
  float z[4][2][1], bz[4][2];
  lstm_bias_pair<NH>(b_, j0, bz);
  wave_sync();
  const float* const xr[1] = {xo + g * r.XS};
  const float* const hr[1] = {hp};
  lstm_gates_valu<NH, 1>(NT->wx, NT->wh, D, xr, hr, lane, z);
#pragma unroll
  for (int u = 0; u < 2; u++) {
    const int j = j0 + u;
    const LstmCell cl = lstm_cell(z[0][u][0], z[1][u][0], z[2][u][0], z[3][u][0], bz[0][u], bz[1][u] + fb, bz[2][u], bz[3][u], cp[u]);
    lstm_state_store<NH>(sp, j, cl);                                                // agent g's state after its step
    hn[j] = cl.hn;
  }
  wave_sync();
  float m[1];
  lstm_heads_valu<NH, 1>(NT->head_w, NT->head_w, A, hn, lane, m);   // (lane 16's value sum reads head_w: the value head stays unread)
  const float mean = m[0] + (ok ? pt_global(NT->head_b)[lane] : 0.0f);
  act = mean;
  if (r.noise0) {
    const float ls = ok ? pt_global(NT->logstd)[lane] : 0.0f;
    const float nz = ok ? pt_global(g ? r.noise1 : r.noise0)[policy_noise_index(a, e, s, A, lane)] : 0.0f;
    (void)gauss_row(mean, expf(ls), 0.0f, ok, true, nz, act, A);
  }
  wave_sync();   // the latent rows are rewritten by whatever acts next
}

// LSTM match policy phase (sumo_match_steps_lstm, POLICY 3): match_lstm_side for both agents, nets idx0[e] / idx1[e] (an index outside
// [0, nsnap) raises the abort flag and plays net 0 instead).  No cross-scoring, nothing recorded.
// LDS (floats, from lds_off): x [2][XS] | previous latent [NH] | new latent [NH].
template <int NH, class C, class SA, class RA>
__device__ __forceinline__ void rollout_policy_phase_match_lstm(C& c, const SA& a, const RA& r, int e, int s) {
  const int lane = c.lane;
  float* xo = (float*)(c.sm + r.lds_off);
  float* hp = xo + 2 * r.XS;
  policy_load_obs<true, false>(a, r, e, lane, xo, r.lnet.ob_dim, r.XS);
  const unsigned dn = policy_prev_done(a, e);
  int jn[2];
  policy_snapshot_rows(a, r, e, lane, jn[0], jn[1]);
  float act[2];
#pragma unroll
  for (int g = 0; g < 2; g++) match_lstm_side<NH>(a, r, e, s, lane, g, jn[g], dn, xo, hp, hp + NH, act[g]);
  if (lane < r.lnet.ac_dim) policy_commit_actions<false>(c, a, r, e, lane, act[0], act[1]);
  wave_sync();
}

// One side of a match played by MLP(64,64) checkpoints: agent g in {0, 1} acts with checkpoint idx_g[e] of snaps [nsnap][P] on the raw
// tile (row g acts), mean or mean + exp(logstd) * noise_g as rollout_policy_phase_match.  g = 0 (a literal) is agent 0 of the matches
// against policy-zoo nets (POLICY 5 / 6); the cross-family matches (POLICY 13) pass the seat the launch gives the MLP checkpoints, a
// scalar.  xbuf: [2][XS] | h1 [2][PT_HS] | h2 [2][PT_HS]; column i where ok.
template <class SA, class RA>
__device__ __forceinline__ float match_mlp_side(const SA& a, const RA& r, int e, int s, int lane, int g, int i, bool ok, float* xbuf) {
  const int D = r.L.D, A = r.L.A, XS = r.XS;
  float* h1 = xbuf + 2 * XS;
  float* h2 = h1 + 2 * PT_HS;
  const int j0 = policy_checked_row(a, lane, pt_global(g ? r.idx1 : r.idx0)[e], r.nsnap);
  const float PT_GAS* p0 = pt_global(r.snaps) + (size_t)j0 * r.L.P;
  const f32x4 m0 = trunk_forward<false, 2>(pi_net((const float*)p0, r.L), xbuf, XS, D, h1, h2, lane);
  const float mean = g ? m0[1] : m0[0];
  float act0 = mean;
  if (r.noise0) {
    const float ls0 = ok ? p0[r.L.logstd + i] : 0.0f;
    const float n0 = ok ? pt_global(g ? r.noise1 : r.noise0)[policy_noise_index(a, e, s, A, i)] : 0.0f;
    (void)gauss_row(mean, expf(ls0), 0.0f, ok, true, n0, act0, A);
  }
  return act0;
}

// Agent 1 played by policy-zoo MLP nets (POLICY 5 / 14): zoo net idx1[e] of the table zm on the tile, which is filtered in place (the
// caller has finished every read of the raw rows); noise1, or the mean where noise0 is NULL.  xbuf as match_mlp_side; column i where ok.
template <class SA, class RA>
__device__ __forceinline__ float zoo_mlp_act(const SA& a, const RA& r, int e, int s, int lane, int i, bool ok, float* xbuf, int A) {
  const auto& t = r.zm;
  const int XS = r.XS;
  float* h1 = xbuf + 2 * XS;
  float* h2 = h1 + 2 * PT_HS;
  const int j1 = policy_checked_row(a, lane, pt_global(r.idx1)[e], t.n);
  const float PT_GAS* p1 = pt_global(t.params) + (size_t)j1 * t.L.P;
  const f32x4 m1 = zoo_trunk_forward<2>(pi_net((const float*)p1, t.L), t.filt + (size_t)j1 * 2 * t.D, t.clip, xbuf, XS, t.D, h1, h2, lane);
  float act1 = m1[1];
  if (r.noise0) {
    const float ls1 = ok ? p1[t.L.logstd + i] : 0.0f;
    const float n1 = ok ? pt_global(r.noise1)[policy_noise_index(a, e, s, A, i)] : 0.0f;
    (void)gauss_row(m1[1], expf(ls1), 0.0f, ok, true, n1, act1, A);
  }
  return act1;
}

// Matches against policy-zoo MLP nets (sumo_match_steps_zoo, POLICY 5; the reference's eval_robosumo_against_fix.py:196-230):
// agent 0 through match_mlp_side, agent 1 through zoo_mlp_act (zoo net idx1[e] on the tile filtered in place afterwards).  Noise, score
// counters and quota as sumo_match_steps.
template <class C, class SA, class RA>
__device__ __forceinline__ void rollout_policy_phase_match_zoo(C& c, const SA& a, const RA& r, int e, int s) {
  const int lane = c.lane, i = lane & 15, kq = lane >> 4;
  const int D = r.L.D, A = r.L.A, XS = r.XS;
  float* xbuf = (float*)(c.sm + r.lds_off);        // [2][XS] | h1 [2][PT_HS] | h2 [2][PT_HS]
  policy_load_obs<false, false>(a, r, e, lane, xbuf, D, XS);
  wave_sync();
  const bool ok = i < A && kq == 0;                 // rows 0 and 1 live in the first 16 lanes (D layout: rows 4 kq + r)
  const float act0 = match_mlp_side(a, r, e, s, lane, 0, i, ok, xbuf);
  wave_sync();   // the raw tile is filtered in place
  const float act1 = zoo_mlp_act(a, r, e, s, lane, i, ok, xbuf, A);
  if (ok) policy_commit_actions<false>(c, a, r, e, i, act0, act1);
  wave_sync();   // the action buffer is read back by the env step (other lanes), the scratch region becomes the mass matrix again
}

// Mean of the Gaussian head of zoo LSTM net row p of table t (policy_zoo LSTMPolicy, policy.py:94-199; ZooLSTMPolicy.act's policy
// branch -- the value branch v/emb, lstmv is never evaluated) on ONE staged observation row: observation filter on the first t.D
// columns of xrow (filtered in place), relu embedding (t.D -> 64), BasicLSTMCell(64) in gate order i,j,f,o with the table's forget
// bias, head.  Embedding, gate sums, cell and head run through zoo_lstm_embed / lstm_gates_valu / lstm_cell / lstm_heads_valu in the
// accumulation order of ppo_lstm_step_kernel<64, PPO_LSTM_GATES_IJFO>: every number equals that kernel bit for bit.  Parameter row:
// emb_w [D][64] | emb_b [64] | kernel [64 + 64][256] (input rows, then recurrent rows) | bias [256] | head_w [64][A] | head_b [A] |
// logstd [A].  STATE: the previous state is the row sp (c | h) masked by `keep`, and the new state is written back to it (hand-over
// accesses: the row crosses waves); otherwise the cell starts from zeros and nothing is written -- the recurrent half of the gate
// sum still runs, over a zero row, so the additions stay the step kernel's.  sc: embedding [64] | previous latent [64] | new latent
// [64] (16-byte aligned LDS).  Lanes < A return their column.
template <bool STATE, class ZT>   // ZT: ZooLstmTable as the launch arguments hold it (constant address space)
__device__ __forceinline__ float zoo_lstm_mean(const ZT& t, const float PT_GAS* p, const float* filt, float* sp, float keep,
                                               float* xrow, float* sc, int lane) {
  constexpr int NH = 64, EM = PT_H;
  const int Dz = t.D, A = t.A;
  const float PT_GAS* emb_b = p + Dz * EM;
  const float PT_GAS* wx = emb_b + EM;
  const float PT_GAS* wh = wx + EM * 4 * NH;
  const float PT_GAS* b_ = wh + NH * 4 * NH;
  const float PT_GAS* head_w = b_ + 4 * NH;
  const float PT_GAS* head_b = head_w + NH * A;
  float *eb = sc, *hp = sc + EM, *hn = hp + NH;
  float cp = 0.0f, hv = 0.0f;
  if constexpr (STATE) { cp = hand_load<true>(sp + lane) * keep; hv = hand_load<true>(sp + NH + lane) * keep; }   // lane owns the unit `lane`
  hp[lane] = hv;
  float bz[4];
#pragma unroll
  for (int g = 0; g < 4; g++) bz[g] = b_[g * NH + lane];       // (in flight during the embedding and the gate sums)
  zoo_lstm_embed(p, emb_b, filt, t.clip, xrow, Dz, eb, lane);
  wave_sync();
  float z[4][1][1];
  const float* const xr[1] = {eb};
  const float* const hr[1] = {hp};
  lstm_gates_valu<NH, 1>((const float*)wx, (const float*)wh, t.emb, xr, hr, lane, z);
  // gate order i, j, f, o: z[1] is the candidate, z[2] the forget gate
  const LstmCell cl = lstm_cell(z[0][0][0], z[2][0][0], z[3][0][0], z[1][0][0], bz[0], bz[2] + t.forget_bias, bz[3], bz[1], cp);
  if constexpr (STATE) lstm_state_store<NH>(sp, lane, cl);
  hn[lane] = cl.hn;
  wave_sync();
  float m[1];
  lstm_heads_valu<NH, 1>((const float*)head_w, (const float*)head_w, A, hn, lane, m);   // (lane 16's value sum reads head_w: no value head here)
  return m[0] + (lane < A ? head_b[lane] : 0.0f);
}

// Agent 1 of the matches against policy-zoo LSTM nets (POLICY 6 / 7): zoo net idx1[e] acts on xrow (agent 1's staged observation) from
// the state row st1[e], which is zeroed first where AGENT 0's done flag of the previous step is set (policy_zoo._evaluate_against
// resets the opponent on done[:, 0]; the rollouts mask with agent 1's flag, so zoo_lstm_mean takes `keep`); noise1, or the mean where
// noise0 is NULL.  Lanes < A return their column of the action.
template <class SA, class RA>
__device__ __forceinline__ float zoo_lstm_act(const SA& a, const RA& r, int e, int s, int lane, unsigned dn, float* xrow, float* sc) {
  const auto& t = r.zl;
  const int A = t.A;
  const int j1 = policy_checked_row(a, lane, pt_global(r.idx1)[e], t.n);
  const float PT_GAS* p = pt_global(t.params) + (size_t)j1 * t.P;
  const float keep = 1.0f - (float)(dn & 0xff);
  const float mean = zoo_lstm_mean<true>(t, p, t.filt + (size_t)j1 * 2 * t.D, r.st1 + (size_t)e * 128, keep, xrow, sc, lane);
  const bool ok = lane < A;
  float act = mean;
  if (r.noise0) {
    const float ls = ok ? p[t.P - A + lane] : 0.0f;   // the row ends with logstd [A]
    const float nz = ok ? pt_global(r.noise1)[policy_noise_index(a, e, s, A, lane)] : 0.0f;
    (void)gauss_row(mean, expf(ls), 0.0f, ok, true, nz, act, A);
  }
  return act;
}

// MLP(64,64) checkpoints against policy-zoo LSTM nets (sumo_match_steps_zoo_lstm, POLICY 6): agent 0 through match_mlp_side; agent 1
// through zoo_lstm_act on row 1 of the tile, its rows in the hidden tiles' place once agent 0's trunk is done (no extra LDS).
template <class C, class SA, class RA>
__device__ __forceinline__ void rollout_policy_phase_match_zoo_lstm(C& c, const SA& a, const RA& r, int e, int s) {
  const int lane = c.lane, i = lane & 15, kq = lane >> 4;
  float* xbuf = (float*)(c.sm + r.lds_off);        // [2][XS] | h1 [2][PT_HS] | h2 [2][PT_HS]
  policy_load_obs<false, false>(a, r, e, lane, xbuf, r.L.D, r.XS);
  const unsigned dn = policy_prev_done(a, e);
  wave_sync();
  const bool ok = i < r.L.A && kq == 0;             // row 0 lives in the first 16 lanes (D layout: rows 4 kq + r)
  const float act0 = match_mlp_side(a, r, e, s, lane, 0, i, ok, xbuf);
  wave_sync();   // the hidden tiles become the cell's rows
  const float act1 = zoo_lstm_act(a, r, e, s, lane, dn, xbuf + r.XS, xbuf + r.zl.sc_off);
  if (ok) policy_commit_actions<false>(c, a, r, e, i, act0, act1);
  wave_sync();   // the action buffer is read back by the env step (other lanes), the scratch region becomes the mass matrix again
}

// LSTM(128) checkpoints against policy-zoo LSTM nets (sumo_match_steps_lstm_zoo_lstm, POLICY 7): agent 0 is side 0 of mode 3
// (match_lstm_side: net idx0[e] of onets); agent 1 through zoo_lstm_act on row 1 of the tile, its rows in the latent rows' place once
// agent 0's head is done.
template <int NH, class C, class SA, class RA>
__device__ __forceinline__ void rollout_policy_phase_match_lstm_zoo_lstm(C& c, const SA& a, const RA& r, int e, int s) {
  const int lane = c.lane;
  float* xo = (float*)(c.sm + r.lds_off);
  float* hp = xo + 2 * r.XS;
  policy_load_obs<true, false>(a, r, e, lane, xo, r.lnet.ob_dim, r.XS);
  const unsigned dn = policy_prev_done(a, e);
  const int jn = policy_checked_row(a, lane, pt_global(r.idx0)[e], r.nsnap);
  float act0;
  match_lstm_side<NH>(a, r, e, s, lane, 0, jn, dn, xo, hp, hp + NH, act0);
  const float act1 = zoo_lstm_act(a, r, e, s, lane, dn, xo + r.XS, xo + r.zl.sc_off);
  if (lane < r.lnet.ac_dim) policy_commit_actions<false>(c, a, r, e, lane, act0, act1);
  wave_sync();
}

// Cross-family checkpoint matches (sumo_match_steps_cross, POLICY 13): agent lstm_side is one side of mode 3 (match_lstm_side: net
// idx_g[e] of onets [nsnap_lstm] on its state row, masked by that agent's done flag of the previous step; st0 == st1 == the one state
// buffer of the launch), the other agent one side of the MLP matches (match_mlp_side: checkpoint idx_g[e] of snaps [nsnap]).  The seat
// is a launch field, read as a scalar: the side functions take it as a value (row of the tile, index / noise / state pointers are
// scalar selects), so there is one body per kernel variant and no branch around the sides.  Each index is checked against its own
// table.  LDS (floats, from lds_off): x [2][XS], zero-padded | previous latent [NH] | new latent [NH], then -- after the wave_sync
// that ends match_lstm_side -- h1 [2][PT_HS] | h2 [2][PT_HS] of the MLP trunk in the same place.
template <int NH, class C, class SA, class RA>
__device__ __forceinline__ void rollout_policy_phase_match_cross(C& c, const SA& a, const RA& r, int e, int s) {
  const int lane = c.lane, i = lane & 15, kq = lane >> 4;
  float* xo = (float*)(c.sm + r.lds_off);
  float* hp = xo + 2 * r.XS;
  policy_load_obs<true, false>(a, r, e, lane, xo, r.lnet.ob_dim, r.XS);
  const unsigned dn = policy_prev_done(a, e);
  const int gl = r.lstm_side;
  const int jn = policy_checked_row(a, lane, pt_global(gl ? r.idx1 : r.idx0)[e], r.nsnap_lstm);
  float actl;
  match_lstm_side<NH>(a, r, e, s, lane, gl, jn, dn, xo, hp, hp + NH, actl);
  const bool ok = i < r.L.A && kq == 0;             // both sides leave their columns in the lanes < A
  const float actm = match_mlp_side(a, r, e, s, lane, 1 - gl, i, ok, xo);
  if (ok) policy_commit_actions<false>(c, a, r, e, i, gl ? actm : actl, gl ? actl : actm);
  wave_sync();   // the action buffer is read back by the env step (other lanes), the scratch region is the step's again
}

// LSTM(128) checkpoints against policy-zoo MLP nets (sumo_match_steps_lstm_zoo, POLICY 14): agent 0 is side 0 of mode 3
// (match_lstm_side: net idx0[e] of onets) on the raw tile; only then agent 1's zoo net filters the tile in place (zoo_mlp_act, agent
// 1 of mode 5), its hidden tiles in the latent rows' place -- the order of mode 9.
template <int NH, class C, class SA, class RA>
__device__ __forceinline__ void rollout_policy_phase_match_lstm_zoo(C& c, const SA& a, const RA& r, int e, int s) {
  const int lane = c.lane, i = lane & 15, kq = lane >> 4;
  const int A = r.lnet.ac_dim;
  float* xo = (float*)(c.sm + r.lds_off);
  float* hp = xo + 2 * r.XS;
  policy_load_obs<true, false>(a, r, e, lane, xo, r.lnet.ob_dim, r.XS);
  const unsigned dn = policy_prev_done(a, e);
  const int jn = policy_checked_row(a, lane, pt_global(r.idx0)[e], r.nsnap);
  float act0;
  match_lstm_side<NH>(a, r, e, s, lane, 0, jn, dn, xo, hp, hp + NH, act0);   // (its last wave_sync: the raw tile is filtered in place)
  const bool ok = i < A && kq == 0;
  const float act1 = zoo_mlp_act(a, r, e, s, lane, i, ok, xo, A);
  if (ok) policy_commit_actions<false>(c, a, r, e, i, act0, act1);
  wave_sync();
}

// ---- rollouts against policy-zoo nets (POLICY 4, 8 .. 12): a learner front, then a zoo pass ----
// What a learner front leaves for the zoo pass and the record: agent 0's sampled action (column of the lane) and its neglogp, the
// learner's mean on row 1 (to score agent 1's action), exp(logstd) / sum(logstd), the values of both rows.
struct LearnerFront { float nlp0, mL1, stdL, sumL, v0, v1, act0; };

// MLP(64,64) learner (POLICY 4, 8, 11): the raw tile (no padding) into LDS and the record, the done flags (returned in dn) into the
// record, policy and value trunks on both rows, agent 0's action sampled.  Heads are indexed by i = lane & 15: rows 0 and 1 live in
// the first 16 lanes (D layout: rows 4 kq + r).  xbuf: [2][XS] | h1 [2][PT_HS] | h2 [2][PT_HS].  Every number equals ppo_forward.
template <class SA, class RA>
__device__ __forceinline__ LearnerFront mlp_learner_front(const SA& a, const RA& r, int e, int s, int lane, float* xbuf, size_t slot0,
                                                          size_t slot1, unsigned& dn) {
  const int i = lane & 15, kq = lane >> 4;
  const int D = r.L.D, A = r.L.A, XS = r.XS;
  float* h1 = xbuf + 2 * XS;
  float* h2 = h1 + 2 * PT_HS;
  policy_load_obs<false, true>(a, r, e, lane, xbuf, D, XS, slot0, slot1);
  dn = policy_prev_done(a, e);
  if (lane < 2) policy_record_done(r, lane, slot0, slot1, dn);
  wave_sync();
  const float PT_GAS* lp = pt_global(r.learner);
  LearnerFront f;
  const f32x4 mL4 = trunk_forward<false, 2>(pi_net((const float*)lp, r.L), xbuf, XS, D, h1, h2, lane);
  const float mL0 = mL4[0];
  f.mL1 = mL4[1];
  wave_sync();
  const f32x4 vL4 = trunk_forward<false, 2>(vf_net((const float*)lp, r.L), xbuf, XS, D, h1, h2, lane);
  f.v0 = vL4[0]; f.v1 = vL4[1];
  const bool colk = i < A;
  const bool ok = colk && kq == 0;
  const float lsL = colk ? lp[r.L.logstd + i] : 0.0f;
  f.stdL = expf(lsL); f.sumL = row16_sum(lsL);
  f.act0 = 0.0f;
  f.nlp0 = gauss_row(mL0, f.stdL, f.sumL, ok, true, ok ? pt_global(r.noise0)[policy_noise_index(a, e, s, A, i)] : 0.0f, f.act0, A);
  return f;
}

// LSTM(128) learner (POLICY 9, 10, 12): the zero-padded tile and the done flags as above, then two evaluations in one pass over the
// learner's weights:
//   row C = (obs 0, agent 0's state)  -> action 0, neglogp, value, agent 0's new state   (row C of rollout_policy_phase_lstm)
//   row E = (obs 1, zero state)       -> the learner's likelihood AND value of action 1  (its row E; there is no row D: a zoo net's
//                                        state is not the learner's, so the zero-state evaluation also values)
// Heads are indexed by the lane (lanes < A).  xo: x [2][XS] | zero row [NH] | agent 0's previous latent [NH] | new latents [2][NH].
// Every number equals ppo_lstm_step.
template <int NH, class SA, class RA>
__device__ __forceinline__ LearnerFront lstm_learner_front(const SA& a, const RA& r, int e, int s, int lane, float* xo, size_t slot0,
                                                           size_t slot1, unsigned& dn) {
  const auto& NL = r.lnet;
  const int D = NL.ob_dim, A = NL.ac_dim, XS = r.XS;
  float* hz = xo + 2 * XS;
  float* hp = hz + NH;
  float* hn = hp + NH;
  policy_load_obs<true, true>(a, r, e, lane, xo, D, XS, slot0, slot1);
  dn = policy_prev_done(a, e);
  if (lane < 2) policy_record_done(r, lane, slot0, slot1, dn);
  const float keep0 = 1.0f - (float)(dn & 0xff);
  float* s0p = r.st0 + (size_t)e * 2 * NH;
  const int j0 = 2 * lane;                           // lane owns the units 2 lane, 2 lane + 1
  float c0[2];
  lstm_state_pair(s0p + j0, keep0, c0);
  lstm_state_pair(s0p + NH + j0, keep0, hp + j0);
  hz[j0] = 0.0f; hz[j0 + 1] = 0.0f;
  wave_sync();
  const bool ok = lane < A;
  const float fb = NL.forget_bias;
  float z[4][2][2], bz[4][2];
  lstm_bias_pair<NH>(pt_global(NL.b), j0, bz);   // (in flight during the gate sums)
  const float* const xr[2] = {xo, xo + XS};
  const float* const hr[2] = {hp, hz};
  lstm_gates_valu<NH, 2>(NL.wx, NL.wh, D, xr, hr, lane, z);
#pragma unroll
  for (int u = 0; u < 2; u++) {
    const int j = j0 + u;
    const float bi = bz[0][u], bf = bz[1][u] + fb, bo = bz[2][u], bu = bz[3][u];   // gate order i, f, o, u
    const LstmCell cc = lstm_cell(z[0][u][0], z[1][u][0], z[2][u][0], z[3][u][0], bi, bf, bo, bu, c0[u]);
    const LstmCell ce = lstm_cell(z[0][u][1], z[1][u][1], z[2][u][1], z[3][u][1], bi, bf, bo, bu, hz[j]);
    lstm_state_store<NH>(s0p, j, cc);                                              // agent 0's state after the learner's step
    hn[j] = cc.hn; hn[NH + j] = ce.hn;
  }
  wave_sync();
  float m[2];
  lstm_heads_valu<NH, 2>(NL.head_w, NL.vf_w, A, hn, lane, m);
  const float hb = ok ? pt_global(NL.head_b)[lane] : 0.0f, ls = ok ? pt_global(NL.logstd)[lane] : 0.0f;
  LearnerFront f;
  f.stdL = expf(ls); f.sumL = row16_sum(ls);
  const float vb = pt_global(NL.vf_b)[0];
  f.v0 = __shfl(m[0], 16) + vb; f.v1 = __shfl(m[1], 16) + vb;
  f.mL1 = m[1] + hb;
  f.act0 = 0.0f;
  f.nlp0 = gauss_row(m[0] + hb, f.stdL, f.sumL, ok, true, ok ? pt_global(r.noise0)[policy_noise_index(a, e, s, A, lane)] : 0.0f, f.act0, A);
  return f;
}

// The zoo side of a rollout step, once the learner has read the raw tile and sampled act0 (and a wave_sync has passed): the zoo net
// scores agent 0's action on row 0 (onlp0), samples agent 1's on row 1 (act1, onlp1), and the learner scores that one (nlp1).  Column
// i where ok, from the caller's front (ok implies i == lane).  xbuf: x [2][XS] followed by the scratch the pass needs.
// zoo_mlp_pass: row jz of the MLP table -- its tanh trunk of input width zm.D on both rows of the tile, filtered in place
// (zoo_trunk_forward: no second tile; the hidden tiles [2][PT_HS] twice behind the tile); the zoo net's value trunk is not
// evaluated.  Every number equals ppo_forward_filtered.
template <class SA, class RA>
__device__ __forceinline__ void zoo_mlp_pass(const SA& a, const RA& r, int e, int s, int lane, int i, bool ok, int jz, float* xbuf, int A,
                                             const LearnerFront& f, float& act1, float& onlp0, float& onlp1, float& nlp1) {
  const auto& t = r.zm;
  const int XS = r.XS;
  float* h1 = xbuf + 2 * XS;
  float* h2 = h1 + 2 * PT_HS;
  const float PT_GAS* zp = pt_global(t.params) + (size_t)jz * t.L.P;
  const f32x4 mO = zoo_trunk_forward<2>(pi_net((const float*)zp, t.L), t.filt + (size_t)jz * 2 * t.D, t.clip, xbuf, XS, t.D, h1, h2, lane);
  const float lsO = ok ? zp[t.L.logstd + i] : 0.0f;
  const float stdO = expf(lsO), sumO = row16_sum(lsO);
  const float n1 = ok ? pt_global(r.noise1)[policy_noise_index(a, e, s, A, i)] : 0.0f;
  float act0 = f.act0;
  onlp0 = gauss_row(mO[0], stdO, sumO, ok, false, 0.0f, act0, A);        // the zoo net scores agent 0's action
  onlp1 = gauss_row(mO[1], stdO, sumO, ok, true, n1, act1, A);           // the zoo net samples for agent 1 ...
  nlp1 = gauss_row(f.mL1, f.stdL, f.sumL, ok, false, 0.0f, act1, A);     // ... the learner scores it
}

// zoo_lstm_pass: row jz of the LSTM table -- zoo_lstm_mean on row 1 from the env's state row st1[e], masked by AGENT 1's done flag of
// the previous step (the Runner's M = dones[:, 1]) and advanced in place, then on row 0 from a zero state, writing no state (the
// Runner's scoring calls feed no state); cell rows at zl.sc_off, in the place of the learner's hidden tiles / latent rows.  Every
// number equals ppo_lstm_step.
template <class SA, class RA>
__device__ __forceinline__ void zoo_lstm_pass(const SA& a, const RA& r, int e, int s, int lane, int i, bool ok, int jz, unsigned dn,
                                              float* xbuf, int A, const LearnerFront& f, float& act1, float& onlp0, float& onlp1, float& nlp1) {
  const auto& t = r.zl;
  const float PT_GAS* zp = pt_global(t.params) + (size_t)jz * t.P;
  const float* zf = t.filt + (size_t)jz * 2 * t.D;
  float* sc = xbuf + t.sc_off;
  const float lsO = ok ? zp[t.P - A + i] : 0.0f;     // the row ends with logstd [A]
  const float stdO = expf(lsO), sumO = row16_sum(lsO);
  const float n1 = ok ? pt_global(r.noise1)[policy_noise_index(a, e, s, A, i)] : 0.0f;
  const float keep1 = 1.0f - (float)((dn >> 8) & 0xff);
  const float mO1 = zoo_lstm_mean<true>(t, zp, zf, r.st1 + (size_t)e * 128, keep1, xbuf + r.XS, sc, lane);
  onlp1 = gauss_row(mO1, stdO, sumO, ok, true, n1, act1, A);             // the zoo net samples for agent 1 ...
  nlp1 = gauss_row(f.mL1, f.stdL, f.sumL, ok, false, 0.0f, act1, A);     // ... the learner scores it
  wave_sync();   // the cell's rows are rewritten by the scoring pass
  const float mO0 = zoo_lstm_mean<false>(t, zp, zf, nullptr, 0.0f, xbuf, sc, lane);
  float act0 = f.act0;
  onlp0 = gauss_row(mO0, stdO, sumO, ok, false, 0.0f, act0, A);          // the zoo net (zero state) scores agent 0's action
}

// The league entry of env column `col` (r.tile_net per 16-env tile of the whole env set, NULL = entry 0), checked against the two
// tables' sizes like every table row.  One value per wave, so league_zoo_pass branches on it with a scalar branch: entry je is row
// je of the MLP table or row je - zm.n of the LSTM table.
template <class SA, class RA>
__device__ __forceinline__ int league_entry(const SA& a, const RA& r, int lane, size_t col) {
  const int je = policy_checked_row(a, lane, r.tile_net ? pt_global(r.tile_net)[col >> 4] : 0, r.zm.n + r.zl.n);
  return __builtin_amdgcn_readfirstlane(je);
}
template <class SA, class RA>
__device__ __forceinline__ void league_zoo_pass(const SA& a, const RA& r, int e, int s, int lane, int i, bool ok, int je, unsigned dn,
                                                float* xbuf, int A, const LearnerFront& f, float& act1, float& onlp0, float& onlp1, float& nlp1) {
  if (je < r.zm.n) zoo_mlp_pass(a, r, e, s, lane, i, ok, je, xbuf, A, f, act1, onlp0, onlp1, nlp1);
  else zoo_lstm_pass(a, r, e, s, lane, i, ok, je - r.zm.n, dn, xbuf, A, f, act1, onlp0, onlp1, nlp1);
}

// Rollout policy phase of a learner against policy-zoo nets (learn(opponent_mode='fix'), reference alg_ppo.py:194-206):
//   LSTM_LEARNER false: sumo_rollout_steps_zoo / _zoo_lstm / _zoo_league           (POLICY 4 / 8 / 11), zoo row opp_idx[e]
//   LSTM_LEARNER true:  sumo_rollout_steps_lstm_zoo / _lstm_zoo_lstm / _lstm_zoo_league (POLICY 9 / 10 / 12), zoo row tile_net[col >> 4]
//                       per 16-env tile of the whole env set, as the snapshot of mode 1
// A league (ZOO_LEAGUE) takes its entry from tile_net for either learner (league_entry).  The learner
// reads the raw tile first (it is in the record by then); only then the zoo net filters the rows in place and takes over the scratch
// behind the tile.  Heads and record as rollout_policy_phase.
enum { ZOO_MLP, ZOO_LSTM, ZOO_LEAGUE };
template <bool LSTM_LEARNER, int ZOO_KIND, class C, class SA, class RA>
__device__ __forceinline__ void rollout_policy_phase_vs_zoo(C& c, const SA& a, const RA& r, int e, int s) {
  const int lane = c.lane;
  const int i = LSTM_LEARNER ? lane : lane & 15;
  const int A = LSTM_LEARNER ? r.lnet.ac_dim : r.L.A;
  const bool ok = i < A && (LSTM_LEARNER || (lane >> 4) == 0);
  float* xbuf = (float*)(c.sm + r.lds_off);
  const size_t col = (size_t)r.env_offset + e;
  const size_t slot0 = ((size_t)0 * r.T + s) * r.Ntot + col, slot1 = ((size_t)1 * r.T + s) * r.Ntot + col;
  int jz;   // the zoo net of the step: a row of the mode's table, or a league entry
  if constexpr (ZOO_KIND == ZOO_LEAGUE) jz = league_entry(a, r, lane, col);
  else if constexpr (LSTM_LEARNER) jz = policy_checked_row(a, lane, r.tile_net ? pt_global(r.tile_net)[col >> 4] : 0, ZOO_KIND == ZOO_MLP ? r.zm.n : r.zl.n);
  else jz = policy_checked_row(a, lane, r.opp_idx ? pt_global(r.opp_idx)[e] : 0, ZOO_KIND == ZOO_MLP ? r.zm.n : r.zl.n);
  unsigned dn;
  LearnerFront f;
  if constexpr (LSTM_LEARNER) f = lstm_learner_front<128>(a, r, e, s, lane, xbuf, slot0, slot1, dn);
  else f = mlp_learner_front(a, r, e, s, lane, xbuf, slot0, slot1, dn);
  wave_sync();   // the raw tile is filtered in place, the hidden tiles / latent rows become the zoo net's
  float act1 = 0.0f, onlp0, onlp1, nlp1;
  if constexpr (ZOO_KIND == ZOO_MLP) zoo_mlp_pass(a, r, e, s, lane, i, ok, jz, xbuf, A, f, act1, onlp0, onlp1, nlp1);
  else if constexpr (ZOO_KIND == ZOO_LSTM) zoo_lstm_pass(a, r, e, s, lane, i, ok, jz, dn, xbuf, A, f, act1, onlp0, onlp1, nlp1);
  else league_zoo_pass(a, r, e, s, lane, i, ok, jz, dn, xbuf, A, f, act1, onlp0, onlp1, nlp1);
  if (ok) policy_commit_actions<true>(c, a, r, e, i, f.act0, act1, A, slot0, slot1);
  if (lane == 0) policy_record_scalars(r, slot0, slot1, f.nlp0, nlp1, onlp0, onlp1, f.v0, f.v1);
  wave_sync();   // the action buffer is read back by the env step (other lanes), the scratch region is the step's again
}

// ---- co-training on a match-up of two species (POLICY 16, sumo_rollout_steps_pair) ----
// policy_load_obs for two widths: observation g into x row g, zero from D_g to XS; where side g records, its D_g columns also go into
// its record (an exact copy of what was read).
template <class SA, class RA>
__device__ __forceinline__ void policy_load_obs_pair(const SA& a, const RA& r, int e, int lane, float* x, int XS, bool rec0, bool rec1, size_t slot) {
  const float* ob = a.obs + (size_t)e * 2 * a.obs_stride;
  const int D0 = r.pair[0].L.D, D1 = r.pair[1].L.D;
  for (int k = lane; k < XS; k += WAVE) {
    float o0 = 0.0f, o1 = 0.0f;
    if (k < D0) { o0 = hand_load<true>(ob + k); if (rec0) pt_global(r.pair[0].obs)[slot * D0 + k] = o0; }
    if (k < D1) { o1 = hand_load<true>(ob + a.obs_stride + k); if (rec1) pt_global(r.pair[1].obs)[slot * D1 + k] = o1; }
    x[k] = o0; x[XS + k] = o1;
  }
}
// policy_commit_actions for one side of its own width: column i < A_g of agent g's action into the env's action buffer and the step's
// control vector.
template <class C, class SA>
__device__ __forceinline__ void policy_commit_action_side(C& c, const SA& a, int e, int g, int i, float act) {
  float* ae = const_cast<float*>(a.actions) + ((size_t)e * 2 + g) * a.act_stride;
  hand_store<true>(ae + i, act);
  const auto& mdl = model_view(c);
  S(ctrl)[MI(agent_uadr)[g] + i] = (double)act;
}

// gauss_row's neglogp of `act` with its three roundings in the order ppo_forward's kernels have them: c A = 0.5 log(2 pi) * A rounded on
// its own, fma(0.5, ss, c A), then + sum_logstd.  The source expression `0.5f * ss + c * A + sum_logstd` leaves the contraction to the
// compiler, which forms that fma wherever the product c A has several uses (gauss_row called for two or four rows) and
// fma(c, A, 0.5 ss) where it has one -- as in the loop over the sides below, whose neglogp then differed from ppo_forward's in the last bit.
__device__ __forceinline__ float gauss_neglogp_pinned(float m, float std, float sum_logstd, bool ok, float act, int A) {
  const float z = ok ? (act - m) / std : 0.0f;
  const float ss = row16_sum(z * z);
  float cA = 0.5f * PT_LOG2PI_F * (float)A;
  asm volatile("" : "+v"(cA));   // (a value of its own: nothing is contracted into or out of it)
  return __builtin_fmaf(0.5f, ss, cA) + sum_logstd;
}

// Both seats of a co-training step.  Side g plays row tile_row_g[tile] of its table (tile = (env_offset + e) >> 4; a row outside the
// table raises the launch's abort flag and plays row 0, as policy_checked_row does for the zoo modes).  On a RECORDING tile of side g
// (record_row_g < 0, or the tile plays that row: wave-uniform) policy and value trunk run in one pass of mlp_rows_valu<2, 1> on x row g
// and the side's observation, action, neglogp, value and own previous-step done flag go to its record at [s][env_offset + e]; on any
// other tile only the policy trunk runs (mlp_rows_valu<1, 1>) and nothing of the side is recorded.  Every number is ppo_forward's on
// that row and observation, bit for bit (mlp_rows_valu, gauss_row).  LDS (floats, from lds_off): x [2][XS] | activation rows [2][PT_VS].
template <class C, class SA, class RA>
__device__ __forceinline__ void rollout_policy_phase_pair(C& c, const SA& a, const RA& r, int e, int s) {
  const int lane = c.lane, i = lane & 15, kq = lane >> 4;
  const int XS = r.XS;
  float* xbuf = (float*)(c.sm + r.lds_off);
  float* hb = xbuf + 2 * XS;
  const size_t col = (size_t)r.env_offset + e;
  const size_t slot = (size_t)s * r.Ntot + col;
  const int tile = (int)(col >> 4);
  // (scalars, not arrays: the loop over the sides below selects them with its wave-uniform counter)
  const int j0 = r.pair[0].tile_row ? pt_global(r.pair[0].tile_row)[tile] : 0, j1 = r.pair[1].tile_row ? pt_global(r.pair[1].tile_row)[tile] : 0;
  const int row0 = __builtin_amdgcn_readfirstlane(policy_checked_row(a, lane, j0, r.pair[0].nrows));
  const int row1 = __builtin_amdgcn_readfirstlane(policy_checked_row(a, lane, j1, r.pair[1].nrows));
  const bool rec0 = r.pair[0].record_row < 0 || row0 == r.pair[0].record_row, rec1 = r.pair[1].record_row < 0 || row1 == r.pair[1].record_row;
  policy_load_obs_pair(a, r, e, lane, xbuf, XS, rec0, rec1, slot);
  const unsigned dn = policy_prev_done(a, e);
  if (lane == 0 && rec0) pt_global(r.pair[0].done)[slot] = (uint8_t)dn;
  if (lane == 1 && rec1) pt_global(r.pair[1].done)[slot] = (uint8_t)(dn >> 8);
  wave_sync();
#pragma unroll 1
  for (int g = 0; g < 2; g++) {   // (one copy of the two trunk passes: the sides differ in launch fields only)
    const auto& ps = r.pair[g];
    const int D = ps.L.D, A = ps.L.A;
    const bool recg = g ? rec1 : rec0;
    const float PT_GAS* p = pt_global(ps.table) + (size_t)(g ? row1 : row0) * ps.row_stride;
    const bool colk = i < A, ok = colk && kq == 0;   // a head's row lives in the first 16 lanes
    const float ls = colk ? p[ps.L.logstd + i] : 0.0f;   // (requested with the first weight rows)
    const float nz = ok ? pt_global(g ? r.noise1 : r.noise0)[slot * A + i] : 0.0f;
    float mean, value = 0.0f;
    if (recg) {
      const Net nets[2] = {pi_net((const float*)p, ps.L), vf_net((const float*)p, ps.L)};
      float m[2][1];
      mlp_rows_valu<2, 1>(nets, xbuf + g * XS, XS, D, hb, lane, m);
      mean = m[0][0]; value = m[1][0];
    } else {
      const Net nets[1] = {pi_net((const float*)p, ps.L)};
      float m[1][1];
      mlp_rows_valu<1, 1>(nets, xbuf + g * XS, XS, D, hb, lane, m);
      mean = m[0][0];
    }
    float act = 0.0f;
    const float std = expf(ls);
    (void)gauss_row(mean, std, 0.0f, ok, true, nz, act, A);   // the sample; its neglogp follows with the roundings pinned
    const float nlp = gauss_neglogp_pinned(mean, std, row16_sum(ls), ok, act, A);
    if (ok) {
      if (recg) pt_global(ps.act)[slot * A + i] = act;
      policy_commit_action_side(c, a, e, g, i, act);
    }
    if (lane == 0 && recg) { pt_global(ps.nlp)[slot] = nlp; pt_global(ps.val)[slot] = value; }
    wave_sync();   // the activation rows are the next side's; after the second side: the action buffer is read back by the env step (other
                   // lanes), the scratch region becomes the mass matrix again
  }
}

// Match post phase: where agent 0's episode ended in the step, score it from the step's winner flags (info[.][7] bit 0, just
// written by this lane): a win if agent 0 carries the flag, a loss if only agent 1 does, a draw otherwise (timeouts, diverged states)
// -- policy_zoo._evaluate_against's rule.  Counted while wins + losses + draws < quota.
template <class C, class SA, class RA>
__device__ __forceinline__ void rollout_post_phase_match(C& c, const SA& a, const RA& r, int e) {
  SYNC();   // the step's episode record was parked in LDS by lane 0 of the epilogue
  if (c.lane == 0 && ((const int*)(S(stash) + 10))[1]) {
    const double* io = a.info + (size_t)e * 2 * SUMO_INFO_STRIDE;
    const int f0 = (int)hand_load<true>(io + 7), f1 = (int)hand_load<true>(io + SUMO_INFO_STRIDE + 7);
    int* sc = r.score + 3 * e;
    const int w = hand_load<true>(sc), l = hand_load<true>(sc + 1), d = hand_load<true>(sc + 2);
    if (w + l + d < r.quota) {
      const int slot = (f0 & 1) ? 0 : ((f1 & 1) ? 1 : 2);
      hand_store<true>(sc + slot, (slot == 0 ? w : slot == 1 ? l : d) + 1);
    }
  }
}

template <class C, class SA, class RA>
__device__ __forceinline__ void rollout_post_phase(C& c, const SA& a, const RA& r, int e, int s) {
  SYNC();   // the step's reward inputs and episode record were parked in LDS by lane 0 of the epilogue
  const int lane = c.lane;
  const size_t col = (size_t)r.env_offset + e;
  if (lane < 2) {   // runner.py:134 + monitor.py:63-78 harvest, as ppo_post_step_kernel
    const double* sh = S(stash) + 5;
    pt_global(r.rew)[((size_t)lane * r.T + s) * r.Ntot + col] = reward_mix(r.alpha, sh[2 * lane], sh[2 * lane + 1]);
    if (lane == 0) {
      const size_t t = (size_t)s * r.Ntot + col;
      const int* rec = (const int*)(sh + 5);
      pt_global(r.ep_done)[t] = (uint8_t)rec[1]; pt_global(r.ep_r)[t] = sh[4]; pt_global(r.ep_l)[t] = rec[0];
    }
  }
}

// The launch arguments are re-read through a laundered pointer in every iteration: accessed as ordinary by-value kernel
// arguments their loads are loop-invariant, get hoisted out of the step loop and stay live across the twenty forward-dynamics
// evaluations of every step (the kernel sits exactly at its 256-register budget).  The pointer addresses the kernel-argument
// segment itself, where the runtime has placed the struct at launch (no separate copy to keep alive).
struct RolloutLaunch { StepArgs a; RolloutArgs r; };
static_assert(sizeof(const Params*) + sizeof(RolloutLaunch) <= 4096, "the launch arguments fit the 4 KB kernel-argument segment");

// Scheduling: the launch is a set of persistent waves (one per wave slot of the chip) that draw TICKETS from a global counter;
// ticket t is step t / N of env t % N.  Env steps differ in cost by 3x (contacts, Newton iterations, agents wrestling), so
// binding a wave to one env for the whole launch leaves a fifth of the slots idle behind the slowest envs (measured: 40-step
// wave lifetimes of 34 ms mean, 50 ms max); with tickets a wave that drew a long step simply draws fewer of them.  A step needs
// its env's previous step: prog[e] counts the finished steps of env e, the wave that draws (e, k) waits for prog[e] == k
// (rarely: that ticket was handed out N tickets earlier).  Dependencies only point to earlier tickets, which are held by waves
// that are already running, so the scheme cannot deadlock whatever the number of resident waves; every wave leaves when the
// tickets run out.  Hand-over of an env between waves: the few hundred bytes that cross (hand_load / hand_store above) go
// through sc1 accesses, the writer drains them (s_waitcnt vmcnt(0)) before its relaxed agent-scope store of prog[e], the
// next wave polls prog[e] with one lane and then reads the record with sc1 loads.  The wait is bounded: a wave that saw no progress for ~2 s raises the
// launch's abort flag (counted in sumo_stats[9]) and every wave drains.
#define ROLLOUT_SPIN_LIMIT (1u << 22)   /* polls of ~0.5 us each */

// POLICY selects the policy phase (and with it the post phase: rollout record, or the score counters of the match modes 2, 3, 5-7, 13, 14):
//    0  sumo_rollout_steps                  MLP(64,64) self-play                      rollout_policy_phase
//    1  sumo_rollout_steps_lstm             LSTM(128) self-play, shared value head    rollout_policy_phase_lstm
//    2  sumo_match_steps                    MLP checkpoint matches                    rollout_policy_phase_match
//    3  sumo_match_steps_lstm               LSTM(128) checkpoint matches              match_lstm_side for both agents
//    4  sumo_rollout_steps_zoo              MLP learner  vs zoo MLP nets              mlp_learner_front  + zoo_mlp_pass
//    5  sumo_match_steps_zoo                MLP checkpoints vs zoo MLP nets           match_mlp_side(0)  + zoo_mlp_act
//    6  sumo_match_steps_zoo_lstm           MLP checkpoints vs zoo LSTM nets          match_mlp_side(0)  + zoo_lstm_act
//    7  sumo_match_steps_lstm_zoo_lstm      LSTM(128) checkpoints vs zoo LSTM nets    match_lstm_side(0) + zoo_lstm_act
//    8  sumo_rollout_steps_zoo_lstm         MLP learner  vs zoo LSTM nets             mlp_learner_front  + zoo_lstm_pass
//    9  sumo_rollout_steps_lstm_zoo         LSTM learner vs zoo MLP nets              lstm_learner_front + zoo_mlp_pass
//   10  sumo_rollout_steps_lstm_zoo_lstm    LSTM learner vs zoo LSTM nets             lstm_learner_front + zoo_lstm_pass
//   11  sumo_rollout_steps_zoo_league       MLP learner  vs a league of both families mlp_learner_front  + league_zoo_pass
//   12  sumo_rollout_steps_lstm_zoo_league  LSTM learner vs a league of both families lstm_learner_front + league_zoo_pass
//   13  sumo_match_steps_cross              MLP checkpoints vs LSTM(128) checkpoints  match_lstm_side(g) + match_mlp_side(1 - g)
//   14  sumo_match_steps_lstm_zoo           LSTM(128) checkpoints vs zoo MLP nets     match_lstm_side(0) + zoo_mlp_act
//   15  sumo_rollout_steps_lstm_reuse       LSTM(128) self-play, agent 1 scored and   rollout_policy_phase_lstm<128, true>
//                                           valued from the learner's shadow state
//   16  sumo_rollout_steps_pair             two MLP seats of their own widths (mixed  rollout_policy_phase_pair
//                                           match-ups), each recording on its tiles
// (4, 8 .. 12 are rollout_policy_phase_vs_zoo<LSTM_LEARNER, ZOO_KIND>.)  The integers are part of the kernels' mangled names, which
// profiles/ and tools/ refer to.  SL 1 / 2: static Layout.
template <int NV, int POLICY, int SL = 0>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(SUMO_WPE_OF(NV), SUMO_WPE_OF(NV))))
sumo_rollout_kernel(const Params* P, RolloutLaunch launch_args) {
  // `launch_args` is read in place from the kernel-argument segment (second argument, 8-byte aligned right behind P) through a
  // pointer the loop launders per ticket -- see the note above RolloutLaunch
  (void)launch_args;
  typedef const RolloutLaunch PT_CAS* LaunchPtr;   // constant address space: every field read is a scalar load
  const LaunchPtr LP = (LaunchPtr)((const char PT_CAS*)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(const Params*));
  Ctx<NV, typename LayoutSel<SL>::type> c;
  ctx_init(c, P, smem_dyn);
  for (;;) {
    LaunchPtr lp = launder_sptr(LP);
    int* sched = lp->r.sched;                      // [0] ticket counter, [1] abort flag, [2 + e] finished steps of env e
    const int N = lp->a.N;
    int t = 0;
    if (c.lane == 0) {
      t = __hip_atomic_fetch_add(sched, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__hip_atomic_load(sched + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) t = 0x7FFFFFFF;   // launch aborted: drain
    }
    t = __builtin_amdgcn_readfirstlane(t);
    if (t >= N * lp->r.K) break;
    int e = t % N, k = t / N;
    if (k > 0) {
      int ok = 1;
      if (c.lane == 0) {
        unsigned spins = 0;
        while (__hip_atomic_load(sched + 2 + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < k) {
          __builtin_amdgcn_s_sleep(16);
          if (++spins > ROLLOUT_SPIN_LIMIT || __hip_atomic_load(sched + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { ok = 0; break; }
        }
        if (!ok) __hip_atomic_store(sched + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      ok = __builtin_amdgcn_readfirstlane(ok);
      if (!ok) { if (c.lane == 0 && lp->a.stats) atomicAdd(lp->a.stats + 9, 1ull); break; }
      asm volatile("" ::: "memory");   // the env's record is read after the poll, through sc1 loads (hand_load): nothing to invalidate
    }
    __builtin_amdgcn_s_setprio(0);   // a wave that raised its issue priority for a dense-solver step (forward()) starts the next ticket level
    // (e, k) wait in LDS during the phases (nothing but the context stays live across the forward-dynamics evaluations)
#ifdef SUMO_DBG_POISON_LDS
    poison_lds(P, c.lane);
#endif
    if (c.lane == 0) { int* tk = (int*)(S(stash) + 4); tk[0] = e; tk[1] = k; }
    lp = launder_sptr(LP);
    int s = lp->r.s0 + k;
    // development (sumo_debug_trace): per-env phase clock, accumulated with atomics (an env's steps run on many waves);
    // the caller zeroes the buffer: [4e] first start, [4e+1] last end, [4e+2] ticks in policy phases, [4e+3] ticks in env steps
    unsigned long long* prof = lp->r.prof;
    unsigned long long t0 = 0;
    if (prof && c.lane == 0) { t0 = wall_clock64(); if (k == 0) atomicExch(prof + PROF_STRIDE * e, t0); }
#ifdef SUMO_DBG_DUMP
    c.dbg = (e == 0 && k == 0) ? lp->a.dbg_qacc : nullptr;
    if (c.dbg) c.st_forward = 0;
#endif
    if constexpr (POLICY == 1) rollout_policy_phase_lstm<128>(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 2) rollout_policy_phase_match(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 3) rollout_policy_phase_match_lstm<128>(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 4) rollout_policy_phase_vs_zoo<false, ZOO_MLP>(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 5) rollout_policy_phase_match_zoo(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 6) rollout_policy_phase_match_zoo_lstm(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 7) rollout_policy_phase_match_lstm_zoo_lstm<128>(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 8) rollout_policy_phase_vs_zoo<false, ZOO_LSTM>(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 9) rollout_policy_phase_vs_zoo<true, ZOO_MLP>(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 10) rollout_policy_phase_vs_zoo<true, ZOO_LSTM>(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 11) rollout_policy_phase_vs_zoo<false, ZOO_LEAGUE>(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 12) rollout_policy_phase_vs_zoo<true, ZOO_LEAGUE>(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 13) rollout_policy_phase_match_cross<128>(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 14) rollout_policy_phase_match_lstm_zoo<128>(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 15) rollout_policy_phase_lstm<128, true>(c, lp->a, lp->r, e, s);
    else if constexpr (POLICY == 16) rollout_policy_phase_pair(c, lp->a, lp->r, e, s);
    else rollout_policy_phase(c, lp->a, lp->r, e, s);
#ifdef SUMO_DBG_HARD_BARRIER
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
    prof = launder_sptr(LP)->r.prof;
    if (prof && c.lane == 0) { const unsigned long long t1 = wall_clock64(); atomicAdd(prof + PROF_STRIDE * e + 2, t1 - t0); S(stash)[11] = __longlong_as_double((long long)t1); }
    env_step_body<true>(c, launder_sptr(LP)->a, e);
    SYNC();
    { const int* tk = (const int*)(S(stash) + 4); e = __builtin_amdgcn_readfirstlane(tk[0]); k = __builtin_amdgcn_readfirstlane(tk[1]); }
    asm volatile("" : "+s"(e), "+s"(k));
    lp = launder_sptr(LP);
    s = lp->r.s0 + k;
    if constexpr (POLICY == 2 || POLICY == 3 || (POLICY >= 5 && POLICY <= 7) || POLICY == 13 || POLICY == 14) rollout_post_phase_match(c, lp->a, lp->r, e);
    else rollout_post_phase(c, lp->a, lp->r, e, s);
    prof = lp->r.prof;
    if (prof && c.lane == 0) {
      const unsigned long long t2 = wall_clock64(), t1 = (unsigned long long)__double_as_longlong(S(stash)[11]);
      atomicAdd(prof + PROF_STRIDE * e + 3, t2 - t1); atomicMax(prof + PROF_STRIDE * e + 1, t2);
    }
    // hand the env over: every sc1 store of the step has reached memory (vmcnt = 0), then the progress counter
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (c.lane == 0) __hip_atomic_store(launder_sptr(LP)->r.sched + 2 + e, k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  flush_stats(c, launder_sptr(LP)->a.stats);
}

// Number of POLICY values above; rollout_launch's table and the instantiation lists below cover 0 .. SUMO_N_POLICY - 1.
#define SUMO_N_POLICY 17
// ---- building in parallel.  The instantiations of sumo_rollout_kernel (7 variants x SUMO_N_POLICY) are most of this file's compile
// time, and one translation unit compiles on one core.  build.py therefore compiles this file several times side by side and links
// the objects into one library:
//   -DSUMO_ROLLOUT_SHARD=k (k = 0 .. 4)  device code of the dynamic-layout rollout kernels <28 + 4 k, *, 0> only (explicit
//                                        instantiations, no host side)
//   -DSUMO_ROLLOUT_EXTERN                everything else; those rollout kernels are declared `extern template`
// The static-layout rollout kernels <28, *, 1> and <44, *, 2> stay in the main object: compiled apart from the step kernels
// of their layout they come out with a different register allocation and schedule (the out-of-line device functions they share
// are specialised per module), and <28, 0, 1> is the benchmark's kernel.  The dynamic-layout ones are the same text in a shard as
// in one translation unit but for PC-relative immediates.
// With neither macro the file is one self-contained translation unit, as the development tools compile it. ----
#if defined(SUMO_ROLLOUT_SHARD) || defined(SUMO_ROLLOUT_EXTERN)
#define SUMO_RK(KW, NV, SL, P) KW template __global__ void sumo_rollout_kernel<NV, P, SL>(const Params*, RolloutLaunch);
#define SUMO_RK_ALL(KW, NV, SL)                                                                                                   \
  SUMO_RK(KW, NV, SL, 0) SUMO_RK(KW, NV, SL, 1) SUMO_RK(KW, NV, SL, 2) SUMO_RK(KW, NV, SL, 3) SUMO_RK(KW, NV, SL, 4)              \
  SUMO_RK(KW, NV, SL, 5) SUMO_RK(KW, NV, SL, 6) SUMO_RK(KW, NV, SL, 7) SUMO_RK(KW, NV, SL, 8) SUMO_RK(KW, NV, SL, 9)              \
  SUMO_RK(KW, NV, SL, 10) SUMO_RK(KW, NV, SL, 11) SUMO_RK(KW, NV, SL, 12) SUMO_RK(KW, NV, SL, 13) SUMO_RK(KW, NV, SL, 14)         \
  SUMO_RK(KW, NV, SL, 15) SUMO_RK(KW, NV, SL, 16)
static_assert(SUMO_N_POLICY == 17, "extend SUMO_RK_ALL");
#ifdef SUMO_ROLLOUT_EXTERN
SUMO_RK_ALL(extern, 28, 0) SUMO_RK_ALL(extern, 32, 0) SUMO_RK_ALL(extern, 36, 0) SUMO_RK_ALL(extern, 40, 0) SUMO_RK_ALL(extern, 44, 0)
#elif SUMO_ROLLOUT_SHARD == 0
SUMO_RK_ALL(, 28, 0)
#elif SUMO_ROLLOUT_SHARD == 1
SUMO_RK_ALL(, 32, 0)
#elif SUMO_ROLLOUT_SHARD == 2
SUMO_RK_ALL(, 36, 0)
#elif SUMO_ROLLOUT_SHARD == 3
SUMO_RK_ALL(, 40, 0)
#elif SUMO_ROLLOUT_SHARD == 4
SUMO_RK_ALL(, 44, 0)
#else
#error "SUMO_ROLLOUT_SHARD: 0 .. 4"
#endif
#endif

#ifndef SUMO_ROLLOUT_SHARD   // a shard object is the device code above and nothing else (DESIGN.md sections 19, 27)
#include "engine_host_scene.h"
#include "engine_host_api.h"
#include "engine_host_fused.h"
#include "engine_host_debug.h"
#endif   // !SUMO_ROLLOUT_SHARD
