// ppo_tile.h -- device pieces shared by the PPO kernels (ppo_kernels.hip) and the fused rollout kernel of the env engine
// (sumo_engine.hip): the flat parameter layout of the MLP(64,64) policy / value nets (reference model.py:153-177 order) and the
// one-wave, one-16-row-tile trunk forward + Gaussian head on v_mfma_f32_16x16x4_f32.  Every kernel that evaluates a net goes
// through these functions, so their outputs agree bit for bit (tests: test_selfplay_forward_equals_separate_evaluations,
// test_rollout_kernel_matches_stepwise_path).
#ifndef PPO_TILE_H
#define PPO_TILE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PT_H 64           /* hidden units (PPO_HIDDEN) */
#define PT_HS 66          /* LDS row stride of a 16 x 64 activation tile (== 2 mod 32) */
#define PT_MAXA 16        /* action dims are padded to one 16-column MFMA tile */
#define PT_LOG2PI_F 1.8378770664093453f
#define PT_WAVE 64

typedef float f32x4 __attribute__((ext_vector_type(4)));

#ifndef PT_PROBE          /* development hooks inside trunk_forward (the rollout kernel's probe build defines them) */
#define PT_PROBE_INIT() do { } while (0)
#define PT_PROBE(k) do { } while (0)
#endif

// Global-memory pointers.  A pointer the compiler cannot trace to a kernel argument (one read from a struct in memory: a net
// description, the laundered launch arguments of the rollout kernel) is a GENERIC pointer and its loads are flat_load, which
// occupy the LDS counter as well as the vector-memory counter: every wait for an LDS read then also waits for the weight loads in
// flight, and a loop that interleaves both runs one memory round trip per iteration whatever the prefetch depth.  Loads through
// an address_space(1) pointer are global_load (vmcnt only).
#if defined(__HIP_DEVICE_COMPILE__)
#define PT_GAS __attribute__((address_space(1)))
#define PT_CAS __attribute__((address_space(4)))   /* constant memory (the kernel-argument segment): scalar loads */
#else   /* the host pass parses the device functions too, and has no address spaces */
#define PT_GAS
#define PT_CAS
#endif
template <class T> __device__ __forceinline__ const T PT_GAS* pt_global(const T* p) { return (const T PT_GAS*)p; }
template <class T> __device__ __forceinline__ T PT_GAS* pt_global(T* p) { return (T PT_GAS*)p; }
#define PT_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

struct ParamLayout {  // offsets into the flat parameter vector (checkpoint order)
  int D, A, P;
  int pi_w0, pi_b0, pi_w1, pi_b1, vf_w0, vf_b0, vf_w1, vf_b1, pi_w, pi_b, logstd, vf_w, vf_b;
};
static ParamLayout make_layout(int D, int A) {
  ParamLayout L;
  L.D = D; L.A = A;
  int o = 0;
  L.pi_w0 = o; o += D * PT_H; L.pi_b0 = o; o += PT_H; L.pi_w1 = o; o += PT_H * PT_H; L.pi_b1 = o; o += PT_H;
  L.vf_w0 = o; o += D * PT_H; L.vf_b0 = o; o += PT_H; L.vf_w1 = o; o += PT_H * PT_H; L.vf_b1 = o; o += PT_H;
  L.pi_w = o; o += PT_H * A; L.pi_b = o; o += A; L.logstd = o; o += A; L.vf_w = o; o += PT_H; L.vf_b = o; o += 1;
  L.P = o;
  return L;
}
#ifndef SUMO_ROLLOUT_SHARD   // sumo_engine.hip's shard objects hold device code only; its main object defines the symbol
extern "C" int ppo_param_count(int ob_dim, int ac_dim) { return make_layout(ob_dim, ac_dim).P; }
#endif

static int x_stride(int D) {  // LDS row stride of the staged observation tile: >= 16*ceil(D/16), == 2 mod 32
  int cols = ((D + 15) / 16) * 16;
  int s = cols;
  while (s % 32 != 2) s++;
  return s;
}

// ---------------------------------------------------------------------------------------------------------
// shared device pieces: one wave, one 16-row tile, one trunk
// ---------------------------------------------------------------------------------------------------------
struct Net { const float PT_GAS *w0, *b0, *w1, *b1, *w2, *b2; int nout; };

// Ordering point between LDS writes and reads of ONE wave (lanes exchanging a tile through the wave's own LDS region).  The
// hardware executes a wave's LDS instructions in order, so only the compiler has to be held: a wavefront-scope fence.  (A
// workgroup-scope fence also drains the vector-memory counter -- s_waitcnt vmcnt(0) -- i.e. it waits for every global store and
// prefetch in flight, e.g. the rollout records written just before a policy trunk.)
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

// forward of one trunk on the staged tile.  h1buf/h2buf [16][PT_HS] receive the relu activations; returns the head tile
// (D layout: lane (i = lane&15, kq = lane>>4) holds rows 4kq+r, column i; columns >= nout are zero + garbage-free).
// ROWS < 16: only the first ROWS rows of the tile carry data (the fused rollout kernel evaluates its env's two observations);
// the buffers then hold ROWS rows, the other rows of the MFMA operands are zero and their results are dropped.  Rows of a
// tile never mix, so a row's result does not depend on ROWS.
template <bool TANH = false, int ROWS = 16>
__device__ __forceinline__ f32x4 trunk_forward(const Net& net, const float* xbuf, int XS, int D, float* h1buf, float* h2buf, int lane) {
  const int i = lane & 15, kq = lane >> 4;
  const int Dp = (D + 3) & ~3;
  f32x4 acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ct++) acc[ct] = (f32x4){0, 0, 0, 0};
  // the biases of all three layers are requested first: read where they are used, each sat behind its own memory round trip
  // (load, wait, add -- per column tile and layer: the compiler does not move a load across the row-guard branches around the
  // activation stores), which was most of the phase's time in the rollout kernel
  float bias0[4], bias1[4];
#pragma unroll
  for (int ct = 0; ct < 4; ct++) { bias0[ct] = net.b0[ct * 16 + i]; bias1[ct] = net.b1[ct * 16 + i]; }
  const bool col_ok = i < net.nout;
  const float bias2 = net.b2[col_ok ? i : 0];
  PT_PROBE_INIT();
  // k-steps are issued eight at a time with all of their operand loads in flight first (32 weight loads per batch): the
  // accumulation order is unchanged, but one memory round trip is exposed per batch instead of one per k-step
  for (int k0 = 0; k0 < Dp; k0 += 32) {
    float a[8], b[8][4];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int k = k0 + 4 * u + kq;
      const bool ok = k < D;
      const int kc = ok ? k : D - 1;   // unconditional loads from a clamped row, zeroed by a select (a guarded load is a branch)
      const float av = xbuf[(ROWS == 16 ? i : (i < ROWS ? i : 0)) * XS + kc];
      a[u] = (ok && (ROWS == 16 || i < ROWS)) ? av : 0.0f;
#pragma unroll
      for (int ct = 0; ct < 4; ct++) { const float wv = net.w0[kc * PT_H + ct * 16 + i]; b[u][ct] = ok ? wv : 0.0f; }
    }
#pragma unroll
    for (int u = 0; u < 8; u++)
      if (k0 + 4 * u < Dp) {
#pragma unroll
        for (int ct = 0; ct < 4; ct++) acc[ct] = PT_MFMA(a[u], b[u][ct], acc[ct]);
      }
  }
  PT_PROBE(0);   // first layer: operand loads + products
#pragma unroll
  for (int ct = 0; ct < 4; ct++) {
    const float bias = bias0[ct];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      float z = acc[ct][r] + bias;
      if (ROWS == 16 || 4 * kq + r < ROWS) h1buf[(4 * kq + r) * PT_HS + ct * 16 + i] = TANH ? tanhf(z) : fmaxf(z, 0.0f);
    }
    acc[ct] = (f32x4){0, 0, 0, 0};
  }
  wave_sync();
  PT_PROBE(1);   // bias + activation + LDS write of the first layer
  {
    float b[PT_H / 4][4];
#pragma unroll
    for (int u = 0; u < PT_H / 4; u++)
#pragma unroll
      for (int ct = 0; ct < 4; ct++) b[u][ct] = net.w1[(4 * u + kq) * PT_H + ct * 16 + i];
    float av[PT_H / 4];   // the tile's A operands in one batch of LDS reads
#pragma unroll
    for (int u = 0; u < PT_H / 4; u++) { const float v = h1buf[(ROWS == 16 ? i : (i < ROWS ? i : 0)) * PT_HS + 4 * u + kq]; av[u] = (ROWS == 16 || i < ROWS) ? v : 0.0f; }
#pragma unroll
    for (int u = 0; u < PT_H / 4; u++) {
#pragma unroll
      for (int ct = 0; ct < 4; ct++) acc[ct] = PT_MFMA(av[u], b[u][ct], acc[ct]);
    }
  }
  PT_PROBE(2);   // second layer: loads + products
#pragma unroll
  for (int ct = 0; ct < 4; ct++) {
    const float bias = bias1[ct];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      float z = acc[ct][r] + bias;
      if (ROWS == 16 || 4 * kq + r < ROWS) h2buf[(4 * kq + r) * PT_HS + ct * 16 + i] = TANH ? tanhf(z) : fmaxf(z, 0.0f);
    }
  }
  wave_sync();
  PT_PROBE(3);   // bias + activation + LDS write of the second layer
  f32x4 out = (f32x4){0, 0, 0, 0};
  {
    float b[PT_H / 4], av[PT_H / 4];
#pragma unroll
    for (int u = 0; u < PT_H / 4; u++) { const float wv = net.w2[(4 * u + kq) * net.nout + (col_ok ? i : 0)]; b[u] = col_ok ? wv : 0.0f; }
#pragma unroll
    for (int u = 0; u < PT_H / 4; u++) { const float v = h2buf[(ROWS == 16 ? i : (i < ROWS ? i : 0)) * PT_HS + 4 * u + kq]; av[u] = (ROWS == 16 || i < ROWS) ? v : 0.0f; }
#pragma unroll
    for (int u = 0; u < PT_H / 4; u++) out = PT_MFMA(av[u], b[u], out);
  }
  PT_PROBE(4);   // head: loads + products
  float bias = col_ok ? bias2 : 0.0f;
#pragma unroll
  for (int r = 0; r < 4; r++) out[r] += bias;
  return out;
}

__device__ __forceinline__ float row16_sum(float v) {  // sum over the 16 lanes that share lane>>4
  v += __shfl_xor(v, 1, PT_WAVE); v += __shfl_xor(v, 2, PT_WAVE); v += __shfl_xor(v, 4, PT_WAVE); v += __shfl_xor(v, 8, PT_WAVE);
  return v;
}
__device__ __forceinline__ float kq_sum(float v) {  // sum over the 4 lanes that share lane&15
  v += __shfl_xor(v, 16, PT_WAVE); v += __shfl_xor(v, 32, PT_WAVE);
  return v;
}

template <class PL>   // ParamLayout in any address space (the rollout kernel reads it in place from its kernel-argument segment)
__device__ __forceinline__ Net pi_net(const float* p_, const PL& L) {
  const float PT_GAS* p = pt_global(p_);
  Net n = {p + L.pi_w0, p + L.pi_b0, p + L.pi_w1, p + L.pi_b1, p + L.pi_w, p + L.pi_b, L.A};
  return n;
}
template <class PL>
__device__ __forceinline__ Net vf_net(const float* p_, const PL& L) {
  const float PT_GAS* p = pt_global(p_);
  Net n = {p + L.vf_w0, p + L.vf_b0, p + L.vf_w1, p + L.vf_b1, p + L.vf_w, p + L.vf_b, 1};
  return n;
}

// The trunks of NT relu nets on R staged rows x [R][XS] on the vector ALU, all nets in one pass, equal bit for bit to NT calls of
// trunk_forward<false, R>: an f32 MFMA adds its four k-products to C as sequential FMAs in ascending k, so a
// lane that owns hidden unit `lane` of every net and runs fmaf over k = 0 .. D-1 from +0 reproduces that column of the tile.  An env
// of the fused rollout has two rows: on a 16-row tile 14 of 16 rows are zero, and the three trunks of a step wait for their weight
// batches one after the other.  Here a k-step is one 256-byte weight row per net (w[k * 64 + lane]), every address is known before
// any data arrives, and ONE ring of four chunks (a chunk = four k-rows of every net; three chunks, 12 NT rows, in flight ahead of
// the products) runs through layer 0 and on through layer 1 of all nets: the layer-1 rows are requested while layer 0 still
// accumulates, the head weights at the hand-over between the layers.
//   x: rows 16-byte aligned (XS a multiple of four, >= (D + 3) & ~3) and ZERO in columns D .. (D + 3) & ~3.  trunk_forward runs
//   its padded k-steps as 0 * 0 products; here the padded steps of the last chunk are 0 * (the clamped row D - 1), which for finite
//   weights adds +-0: that leaves every accumulator alone except -0 (reachable from +0 only through a product that underflows),
//   which 0 * 0 turns into +0 and -0 * w need not.  The `+ 0.0f` behind the loop (only where trunk_forward pads: D & 3) makes
//   both cases +0.  Chunks past (D + 3) / 4 of the last group of four are fetched (clamped rows) and not multiplied.
//   hbuf [NT][R][PT_VS]: the relu activations of layer 0, then of layer 1, cross lanes through it.
//   Heads: the 16-lane group t < NT runs net t's head as lstm_heads_valu does, lane i < nout over the 64 units in ascending order
//   (the k order of trunk_forward's head tile), plus bias; out[t][r] then holds, in EVERY 16-lane group, column i = lane & 15 of
//   row r of net t's head: where trunk_forward's tile has it for the lanes with lane >> 4 == 0 (rows 0, 1 = registers 0, 1).
#define PT_VS 68          /* row stride of hbuf: rows 16-byte aligned, == 4 mod 32 (the head pass reads NT rows at once) */
template <int NT, int R>
__device__ __forceinline__ void mlp_rows_valu(const Net (&net)[NT], const float* x, int XS, int D, float* hbuf, int lane, float (&out)[NT][R]) {
  static_assert(NT >= 1 && NT <= 4, "one 16-lane group per head");
  const int nx = (D + 3) >> 2;        // layer-0 chunks that carry data
  const int g0 = (nx + 3) >> 2;       // groups of four chunks: layer 0, then PT_H / 16 of layer 1
  const int nch = 4 * g0 + PT_H / 4;
  const int i = lane & 15, hg = lane >> 4;
  const float PT_GAS *w0p[NT], *w1p[NT];
  float b0[NT], b1[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) { w0p[t] = net[t].w0; w1p[t] = net[t].w1; b0[t] = net[t].b0[lane]; b1[t] = net[t].b1[lane]; }
  const float PT_GAS *w2p[NT], *b2p[NT];
  int noutp[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) { w2p[t] = net[t].w2; b2p[t] = net[t].b2; noutp[t] = net[t].nout; }
  const float PT_GAS* w2 = w2p[0];
  const float PT_GAS* b2 = b2p[0];
  int nout = noutp[0];
#pragma unroll
  for (int t = 1; t < NT; t++) { const bool mine = hg == t; w2 = mine ? w2p[t] : w2; b2 = mine ? b2p[t] : b2; nout = mine ? noutp[t] : nout; }
  const bool col_ok = hg < NT && i < nout;
  const int hcol = col_ok ? i : 0;
  const float bias2 = b2[hcol];
  float acc[NT][R];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int r = 0; r < R; r++) acc[t][r] = 0.0f;
  auto fetch = [&](int ch, float (&w)[4][NT]) {
    const bool l0 = ch < 4 * g0;
    const int k0 = 4 * (l0 ? ch : ch - 4 * g0), kmax = l0 ? D : PT_H;
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
      int k = k0 + kk;
      if (k >= kmax) k = kmax - 1;   // unconditional loads from a clamped row
#pragma unroll
      for (int t = 0; t < NT; t++) w[kk][t] = (l0 ? w0p[t] : w1p[t])[k * PT_H + lane];
    }
  };
  auto consume0 = [&](int ch, const float (&w)[4][NT]) {   // layer 0: the nets share the x rows (wave-uniform 128-bit LDS reads)
#pragma unroll
    for (int r = 0; r < R; r++) {
      const float4 xv = *(const float4*)(x + r * XS + 4 * ch);
      const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
      for (int kk = 0; kk < 4; kk++)
#pragma unroll
        for (int t = 0; t < NT; t++) acc[t][r] = __builtin_fmaf(xs[kk], w[kk][t], acc[t][r]);
    }
  };
  auto consume1 = [&](int ch, const float (&w)[4][NT]) {   // layer 1: every net on its own activation rows
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int r = 0; r < R; r++) {
        const float4 xv = *(const float4*)(hbuf + (t * R + r) * PT_VS + 4 * ch);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int kk = 0; kk < 4; kk++) acc[t][r] = __builtin_fmaf(xs[kk], w[kk][t], acc[t][r]);
      }
  };
  float w[4][4][NT], w2v[PT_H];
  fetch(0, w[0]); fetch(1, w[1]); fetch(2, w[2]);
  for (int g = 0; g < g0; g++) {
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int ch = 4 * g + b;
      fetch(ch + 3, w[(b + 3) & 3]);
      if (ch < nx) consume0(ch, w[b]);
    }
  }
#pragma unroll
  for (int u = 0; u < PT_H; u++) { const float wv = w2[u * nout + hcol]; w2v[u] = col_ok ? wv : 0.0f; }
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int r = 0; r < R; r++) {
      const float a = (D & 3) ? acc[t][r] + 0.0f : acc[t][r];
      hbuf[(t * R + r) * PT_VS + lane] = fmaxf(a + b0[t], 0.0f);
      acc[t][r] = 0.0f;
    }
  wave_sync();
#pragma unroll
  for (int g = 0; g < PT_H / 16; g++) {
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int c1 = 4 * g + b, nxt = 4 * g0 + c1 + 3;
      fetch(nxt < nch ? nxt : nch - 1, w[(b + 3) & 3]);   // (no branch around the loads: past the end the last chunk is fetched again)
      consume1(c1, w[b]);
    }
  }
  wave_sync();   // every lane has read the layer-0 rows
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int r = 0; r < R; r++) hbuf[(t * R + r) * PT_VS + lane] = fmaxf(acc[t][r] + b1[t], 0.0f);
  wave_sync();
  const float* hrow = hbuf + (hg < NT ? hg : 0) * R * PT_VS;
  const float bias = col_ok ? bias2 : 0.0f;
  float o[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    o[r] = 0.0f;
#pragma unroll
    for (int q = 0; q < PT_H / 4; q++) {
      const float4 hv = *(const float4*)(hrow + r * PT_VS + 4 * q);
      o[r] = __builtin_fmaf(hv.x, w2v[4 * q], o[r]); o[r] = __builtin_fmaf(hv.y, w2v[4 * q + 1], o[r]);
      o[r] = __builtin_fmaf(hv.z, w2v[4 * q + 2], o[r]); o[r] = __builtin_fmaf(hv.w, w2v[4 * q + 3], o[r]);
    }
    o[r] += bias;
  }
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int r = 0; r < R; r++) out[t][r] = __shfl(o[r], 16 * t + i, PT_WAVE);
}

// Policy trunk of a policy-zoo MLP net (policy_zoo MLPPolicy(normalize=True), policy.py:23-91) on ROWS staged rows of x [ROWS][XS]:
// the rows are filtered IN PLACE -- clip((x - mean) * invstd, +-clip) on the first Dz columns, the expression and order of stage_x
// in ppo_kernels.hip; columns Dz .. XS are zeroed -- then the tanh trunk of input width Dz runs on them.  filt: mean [Dz] | 1 / std
// [Dz].  The caller has finished every read of the raw rows (wave_sync before the call); the raw tile is gone afterwards.
template <int ROWS>
__device__ __forceinline__ f32x4 zoo_trunk_forward(const Net& net, const float* filt_, float clip, float* xbuf, int XS, int Dz, float* h1buf,
                                                   float* h2buf, int lane) {
  const float PT_GAS* filt = pt_global(filt_);
  for (int k = lane; k < XS; k += PT_WAVE) {
    const bool cok = k < Dz;
    const float fm = cok ? filt[k] : 0.0f, fi = cok ? filt[Dz + k] : 0.0f;
#pragma unroll
    for (int r = 0; r < ROWS; r++) xbuf[r * XS + k] = cok ? fminf(fmaxf((xbuf[r * XS + k] - fm) * fi, -clip), clip) : 0.0f;
  }
  wave_sync();
  return trunk_forward<true, ROWS>(net, xbuf, XS, Dz, h1buf, h2buf, lane);
}

// One row of the diagonal-Gaussian head (baselines distributions.py:227-251) in the tile's D layout: lane i < A of the row's
// 16-lane group holds the mean m of action dimension i.  sample: act = m + std * noise, else `act` is given.
// Returns -log pi(act | obs) of the row (every lane of the group).
__device__ __forceinline__ float gauss_row(float m, float std, float sum_logstd, bool ok, bool sample, float noise, float& act, int A) {
  if (sample) act = ok ? m + std * noise : m;
  const float z = ok ? (act - m) / std : 0.0f;
  const float ss = row16_sum(z * z);
  return 0.5f * ss + 0.5f * PT_LOG2PI_F * (float)A + sum_logstd;
}

// Gaussian head on a policy tile (D layout): samples (noise != nullptr) or scores `act`; returns the row's neglogp in
// the lanes with i == 0 via nlp[r]
__device__ __forceinline__ void gauss_head(const float* params_, const ParamLayout& L, const f32x4& mean, const float* noise_, int r0, int n,
                                           int lane, float (&act)[4], float (&nlp)[4]) {
  const float PT_GAS* params = pt_global(params_);
  const float PT_GAS* noise = pt_global(noise_);
  const int i = lane & 15, kq = lane >> 4, A = L.A;
  const bool col = i < A;
  const float logstd = col ? params[L.logstd + i] : 0.0f;
  const float std = expf(logstd);
  const float sum_logstd = row16_sum(logstd);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = r0 + 4 * kq + r;
    const bool ok = col && row < n;
    const float nz = (noise && ok) ? noise[(size_t)row * A + i] : 0.0f;
    nlp[r] = gauss_row(mean[r], std, sum_logstd, ok, noise != nullptr, nz, act[r], A);
  }
}

// reward curriculum of the rollout (runner.py:134): alpha * shaping + (1 - alpha) * main, evaluated in float64, stored as float32
__device__ __forceinline__ float reward_mix(double alpha, double shaping, double main_r) {
  return (float)(alpha * shaping + (1 - alpha) * main_r);
}

// ---------------------------------------------------------------------------------------------------------
// recurrent nets (baselines lstm(nlstm), a2c/utils.py:82-103): pieces shared by ppo_lstm_step_kernel (16-row MFMA tiles,
// ppo_kernels.hip) and the fused rollout kernel (an env's few rows on the vector ALU, sumo_engine.hip)
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float pt_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

struct LstmCell { float ig, fg, og, ug, cn, tcn, hn; };
// gate pre-activations (bias not yet added; bf carries the forget-bias offset) and the previous cell -> gates, new cell, latent
__device__ __forceinline__ LstmCell lstm_cell(float zi, float zf, float zo, float zu, float bi, float bf, float bo, float bu, float cp) {
  LstmCell o;
  o.ig = pt_sigmoid(zi + bi); o.fg = pt_sigmoid(zf + bf); o.og = pt_sigmoid(zo + bo); o.ug = tanhf(zu + bu);
  o.cn = __builtin_fmaf(o.fg, cp, o.ig * o.ug);   // one explicit contraction, so every caller rounds alike
  o.tcn = tanhf(o.cn); o.hn = o.og * o.tcn;
  return o;
}

typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));   // two floats at dword alignment (rows of a snapshot pool start at odd offsets)

// Gate pre-activations of R rows on the vector ALU, equal bit for bit to the MFMA tiles of ppo_lstm_step_kernel: an f32 MFMA
// adds its four k-products to C as sequential FMAs in ascending k, so a lane that owns a column and
// runs fmaf over the input block (k = 0 .. D-1) and then the recurrent block (k = 0 .. NH-1) reproduces that column of the
// tile.  One env has 2-3 rows per net: on a 16-row tile 13 of 16 rows would be idle and every B operand a 256-byte load; here a
// lane owns the units 2 lane, 2 lane + 1 -- all four gates of them, columns g NH + 2 lane + {0, 1} -- and a k-step costs four
// 512-byte loads for the whole wave (NH = 64: the unit `lane`, four 256-byte loads).  xr[r] / hr[r]: LDS rows (16-byte aligned; x
// rows zero-padded to a multiple of four).
template <int NH, int R>
__device__ __forceinline__ void lstm_gates_valu(const float* wx, const float* wh, int D, const float* const (&xr)[R], const float* const (&hr)[R],
                                                int lane, float (&z)[4][NH / 64][R]) {
  static_assert(NH == 128 || NH == 64, "two units per lane, or one (NH = 64: the policy-zoo LSTM cell)");
  constexpr int U = NH / 64;   // units per lane; U == 1 keeps the .x half of every weight pair only
  const int nx = (D + 3) >> 2, nch = nx + NH / 4;
  const int col = U * lane;
#pragma unroll
  for (int g = 0; g < 4; g++)
#pragma unroll
    for (int r = 0; r < R; r++) { z[g][0][r] = 0.0f; if constexpr (U == 2) z[g][1][r] = 0.0f; }
  auto fetch = [&](int ch, f32x2u (&w)[4][4]) {
    const bool in_x = ch < nx;
    const float PT_GAS* base = pt_global(in_x ? wx : wh);
    const int k0 = 4 * (in_x ? ch : ch - nx), kmax = in_x ? D : NH;
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
      int k = k0 + kk;
      if (k >= kmax) k = kmax - 1;   // the x rows are zero there: fma(0, w, z) == z for any finite weight
      const float PT_GAS* wrow = base + (size_t)k * 4 * NH + col;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        if constexpr (U == 2) w[kk][g] = *(const f32x2u PT_GAS*)(wrow + g * NH);
        else w[kk][g].x = wrow[g * NH];
      }
    }
  };
  auto consume = [&](int ch, const f32x2u (&w)[4][4]) {
    const bool in_x = ch < nx;
    const int k0 = 4 * (in_x ? ch : ch - nx);
#pragma unroll
    for (int r = 0; r < R; r++) {
      const float4 xv = *(const float4*)((in_x ? xr[r] : hr[r]) + k0);
      const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
      for (int kk = 0; kk < 4; kk++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          z[g][0][r] = __builtin_fmaf(xs[kk], w[kk][g].x, z[g][0][r]);
          if constexpr (U == 2) z[g][1][r] = __builtin_fmaf(xs[kk], w[kk][g].y, z[g][1][r]);
        }
    }
  };
  // a chunk costs one trip to the L2 / MALL (~0.8 us under load) unless enough of them are in flight: ring of four chunk buffers,
  // three chunks (48 loads, 24 KB per wave) ahead of the products
  f32x2u w[4][4][4];
  fetch(0, w[0]); fetch(1, w[1]); fetch(2, w[2]);
  int ch = 0;
  for (; ch + 4 <= nch; ch += 4) {
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int nxt = ch + b + 3;
      fetch(nxt < nch ? nxt : nch - 1, w[(b + 3) & 3]);   // (no branch around the loads: past the end the last chunk is fetched again)
      consume(ch + b, w[b]);
    }
  }
#pragma unroll
  for (int b = 0; b < 3; b++)   // the last nch % 4 chunks are in flight in buffers 0 .. 2
    if (ch + b < nch) consume(ch + b, w[b]);
}

// Input stage of a policy-zoo LSTM net (policy_zoo LSTMPolicy(normalize=True), policy.py:94-199) on ONE staged observation row:
// the row is filtered IN PLACE -- clip((x - mean) * invstd, +-clip) on its first Dz columns, the expression and order of stage_x in
// ppo_kernels.hip -- and the relu embedding (Dz -> 64) goes to erow [64]: lane owns column `lane` and runs fmaf over k = 0 .. Dz - 1
// from zero, the order in which the embedding tiles of ppo_lstm_step_kernel accumulate (an f32 MFMA adds its k-products as
// sequential FMAs in ascending k; its padded k-steps add 0 * 0), then relu(sum + bias).  filt: mean [Dz] |
// 1 / std [Dz]; emb_w [Dz][64], emb_b [64].  The caller orders erow against its readers (wave_sync).
__device__ __forceinline__ void zoo_lstm_embed(const float PT_GAS* emb_w, const float PT_GAS* emb_b, const float* filt_, float clip, float* xrow,
                                               int Dz, float* erow, int lane) {
  const float PT_GAS* filt = pt_global(filt_);
  const float bias = emb_b[lane];
  // Wave-uniform trips and a clamped column instead of `for (k = lane; k < Dz; k += PT_WAVE)`: a lane-strided loop drains EXEC, and in
  // sumo_rollout_kernel<44, 11, 2> the register allocator parked a live value (agent 0's sampled action) in an AGPR right behind that
  // loop's exit, where no lane is active -- the copy wrote nothing and the restore handed back a stale register (DESIGN.md sections 4,
  // 31).  The lanes past Dz recompute column Dz - 1 and store the same value to the same word.
  for (int k0 = 0; k0 < Dz; k0 += PT_WAVE) {
    const int k = k0 + lane < Dz ? k0 + lane : Dz - 1;
    const float y = fminf(fmaxf((xrow[k] - filt[k]) * filt[Dz + k], -clip), clip);
    wave_sync();   // every lane has read its column before column Dz - 1 is rewritten
    xrow[k] = y;
  }
  wave_sync();
  float acc = 0.0f;
  for (int k0 = 0; k0 < Dz; k0 += 16) {   // sixteen 256-byte weight rows in flight per trip to the L2
    float w[16];
#pragma unroll
    for (int u = 0; u < 16; u++) { const int k = k0 + u; w[u] = emb_w[(size_t)(k < Dz ? k : Dz - 1) * PT_H + lane]; }
#pragma unroll
    for (int u = 0; u < 16; u++)
      if (k0 + u < Dz) acc = __builtin_fmaf(xrow[k0 + u], w[u], acc);
  }
  erow[lane] = fmaxf(acc + bias, 0.0f);
}

// Heads on R latent rows in LDS (hn [R][NH]): lane i < A accumulates column i of the Gaussian mean, lane 16 the value, over the
// units in ascending order (the k order of the head tiles of ppo_lstm_step_kernel); biases are added by the caller.
template <int NH, int R>
__device__ __forceinline__ void lstm_heads_valu(const float* head_w_, const float* vf_w_, int A, const float* hn, int lane, float (&acc)[R]) {
  const float PT_GAS* head_w = pt_global(head_w_);
  const float PT_GAS* vf_w = pt_global(vf_w_);
  const bool pi = lane < A, vf = lane == 16;
#pragma unroll
  for (int r = 0; r < R; r++) acc[r] = 0.0f;
  for (int j0 = 0; j0 < NH; j0 += 64) {   // 64 weight loads in flight: two trips to the L2 per head instead of one per 16 units
    float w[64];
#pragma unroll
    for (int u = 0; u < 64; u++) w[u] = pi ? head_w[(j0 + u) * A + lane] : (vf ? vf_w[j0 + u] : 0.0f);
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const float4 hv = *(const float4*)(hn + r * NH + j0 + 4 * q);
        acc[r] = __builtin_fmaf(hv.x, w[4 * q], acc[r]); acc[r] = __builtin_fmaf(hv.y, w[4 * q + 1], acc[r]);
        acc[r] = __builtin_fmaf(hv.z, w[4 * q + 2], acc[r]); acc[r] = __builtin_fmaf(hv.w, w[4 * q + 3], acc[r]);
      }
  }
}

#endif
