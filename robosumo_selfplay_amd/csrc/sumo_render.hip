// sumo_render.hip -- MI355X (gfx950) match renderer (include/sumo_render.h): geom poses from qpos, then an analytic ray caster.
//
// The scene is a few dozen primitives (plane, sphere, capsule, cylinder, box), so a frame is one thread per pixel walking the
// env's geom list.  A block is a 16 x 16 pixel tile of one image (256 threads, four waves); it stages the image's geom records
// (pose, size, type, colour and the camera eye in the geom's frame: 96 B each) into LDS once.  Every lane walks the same list,
// so the type branch is wave-uniform and the LDS reads are same-address broadcasts; only hit or miss differs between lanes.
// float32 arithmetic in forms that do not cancel at arena distances (closest-approach discriminants), plain C++, vector stores.
//
// Poses are forward kinematics as mjcf.kinematics_np states them, in float64, one thread per env, rounded once on store.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/sumo_model.h"
#include "../../include/sumo_render.h"

static thread_local char g_err[256];
extern "C" const char* sumo_render_last_error(void) { return g_err; }
#define FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return code; } while (0)
#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) FAIL(-100, "%s failed: %s", #expr, hipGetErrorString(_e)); } while (0)

#define MAXGEOM SUMO_RENDER_MAXGEOM
#define MAXBODY SUMO_RENDER_MAXBODY
#define TILE 16
#define REC 24   // floats per LDS geom record: centre 0..2, rotation 3..11, size 12..14, type 15 (int bits), colour 16..18, eye in the geom frame 19..21

struct sumo_render {
  int device;
  sumo_model_t hm;            // host view (ibase / fbase point into blob)
  sumo_model_t dm;            // the same offsets over the device copy of the blob
  std::vector<char> blob;
  char* blob_dev;
  float4* gstat_dev;          // [ngeom] size xyz, type as int bits
};

// ---------------------------------------------------------------------------------------------------------------------------------
// poses
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void quat_mul(const double* a, const double* b, double* o) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

__device__ __forceinline__ void quat2mat(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = w * w + x * x - y * y - z * z; R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = w * w - x * x + y * y - z * z; R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = w * w - x * x - y * y + z * z;
}

__device__ __forceinline__ void quat_normalize(double* q) {
  const double s = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] *= s; q[1] *= s; q[2] *= s; q[3] *= s;
}

__device__ __forceinline__ void mat_vec(const double* R, const double* v, double* o) {
  o[0] = R[0] * v[0] + R[1] * v[1] + R[2] * v[2];
  o[1] = R[3] * v[0] + R[4] * v[1] + R[5] * v[2];
  o[2] = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
}

__global__ __launch_bounds__(64) void render_poses_kernel(sumo_model_t m, const double* __restrict__ qpos_all, int n,
                                                          float* __restrict__ poses) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const double* qpos = qpos_all + (size_t)e * m.nq;
  double xpos[MAXBODY][3], xquat[MAXBODY][4];
  xpos[0][0] = xpos[0][1] = xpos[0][2] = 0.0;
  xquat[0][0] = 1.0; xquat[0][1] = xquat[0][2] = xquat[0][3] = 0.0;
  const int32_t *parent = SUMO_I(&m, body_parentid), *jntadr = SUMO_I(&m, body_jntadr), *jntnum = SUMO_I(&m, body_jntnum);
  const int32_t *jtype = SUMO_I(&m, jnt_type), *jqadr = SUMO_I(&m, jnt_qposadr);
  const double *qpos0 = SUMO_F(&m, qpos0), *bpos = SUMO_F(&m, body_pos), *bquat = SUMO_F(&m, body_quat);
  const double *jpos = SUMO_F(&m, jnt_pos), *jaxis = SUMO_F(&m, jnt_axis);
  double R[9], v[3];
  for (int b = 1; b < m.nbody; b++) {
    const int pid = parent[b], ja = jntadr[b], jn = jntnum[b];
    if (jn == 1 && jtype[ja] == SUMO_JNT_FREE) {
      const int qa = jqadr[ja];
      for (int k = 0; k < 3; k++) xpos[b][k] = qpos[qa + k];
      for (int k = 0; k < 4; k++) xquat[b][k] = qpos[qa + 3 + k];
      quat_normalize(xquat[b]);
      continue;
    }
    quat2mat(xquat[pid], R);
    mat_vec(R, bpos + 3 * b, v);
    for (int k = 0; k < 3; k++) xpos[b][k] = xpos[pid][k] + v[k];
    quat_mul(xquat[pid], bquat + 4 * b, xquat[b]);
    for (int j = ja; j < ja + jn; j++) {   // hinge: rotate about jnt_axis by qpos - qpos0, the joint anchor stays where it is
      double anchor[3], ql[4], q[4];
      quat2mat(xquat[b], R);
      mat_vec(R, jpos + 3 * j, v);
      for (int k = 0; k < 3; k++) anchor[k] = xpos[b][k] + v[k];
      const double ang = qpos[jqadr[j]] - qpos0[jqadr[j]];
      const double s = sin(0.5 * ang);
      ql[0] = cos(0.5 * ang); ql[1] = jaxis[3 * j] * s; ql[2] = jaxis[3 * j + 1] * s; ql[3] = jaxis[3 * j + 2] * s;
      quat_mul(xquat[b], ql, q);
      for (int k = 0; k < 4; k++) xquat[b][k] = q[k];
      quat2mat(xquat[b], R);
      mat_vec(R, jpos + 3 * j, v);
      for (int k = 0; k < 3; k++) xpos[b][k] = anchor[k] - v[k];
    }
    quat_normalize(xquat[b]);
  }
  const int32_t* gbody = SUMO_I(&m, geom_bodyid);
  const double *gpos = SUMO_F(&m, geom_pos), *gquat = SUMO_F(&m, geom_quat);
  float* out = poses + (size_t)e * m.ngeom * SUMO_RENDER_POSE_STRIDE;
  for (int g = 0; g < m.ngeom; g++) {
    const int b = gbody[g];
    double q[4];
    quat2mat(xquat[b], R);
    mat_vec(R, gpos + 3 * g, v);
    for (int k = 0; k < 3; k++) out[g * 12 + k] = (float)(xpos[b][k] + v[k]);
    quat_mul(xquat[b], gquat + 4 * g, q);
    quat2mat(q, R);
    for (int k = 0; k < 9; k++) out[g * 12 + 3 + k] = (float)R[k];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// frames
// ---------------------------------------------------------------------------------------------------------------------------------
struct FrameArgs {
  const float *poses, *cams, *colors;
  const float4* gstat;
  uint32_t* rgba;
  float* depth;
  int32_t* id;
  sumo_render_shade shade;
  int n, ncam, ngeom, W, H, tiles_x;
};

// entry of a unit-direction ray o + t d into the sphere of radius r about the origin (closest-approach form: no b*b - c cancellation)
__device__ __forceinline__ bool sphere_entry(float ox, float oy, float oz, float dx, float dy, float dz, float r, float* t) {
  const float b = ox * dx + oy * dy + oz * dz;
  const float lx = ox - b * dx, ly = oy - b * dy, lz = oz - b * dz;
  const float disc = r * r - (lx * lx + ly * ly + lz * lz);
  if (disc < 0.0f) return false;
  *t = -b - sqrtf(disc);
  return true;
}

__global__ __launch_bounds__(TILE * TILE) void render_frames_kernel(FrameArgs a) {
  __shared__ float rec[MAXGEOM * REC];
  const int tid = threadIdx.x;
  const int x = (blockIdx.x % a.tiles_x) * TILE + (tid & (TILE - 1));
  const int y = (blockIdx.x / a.tiles_x) * TILE + (tid >> 4);
  const bool inside = x < a.W && y < a.H;
  const float lx_ = a.shade.light[0], ly_ = a.shade.light[1], lz_ = a.shade.light[2];
  for (int img = blockIdx.y; img < a.n; img += gridDim.y) {   // block-uniform: the barriers below are reached by all threads
    const float* cam = a.cams + (a.ncam == 1 ? 0 : (size_t)img * SUMO_RENDER_CAM_STRIDE);
    const float ex = cam[0], ey = cam[1], ez = cam[2];
    const float* pose = a.poses + (size_t)img * a.ngeom * SUMO_RENDER_POSE_STRIDE;
    for (int i = tid; i < a.ngeom * REC; i += TILE * TILE) {
      const int g = i / REC, k = i - g * REC;
      float v = 0.0f;
      if (k < 12) v = pose[g * 12 + k];
      else if (k < 16) v = ((const float*)a.gstat)[g * 4 + (k - 12)];
      else if (k < 19) v = a.colors[g * 3 + (k - 16)];
      rec[i] = v;
    }
    __syncthreads();
    if (tid < a.ngeom) {   // the eye in the geom's frame: R^T (eye - centre), once per block instead of once per pixel
      float* r = rec + tid * REC;
      const float px = ex - r[0], py = ey - r[1], pz = ez - r[2];
      r[19] = r[3] * px + r[6] * py + r[9] * pz;
      r[20] = r[4] * px + r[7] * py + r[10] * pz;
      r[21] = r[5] * px + r[8] * py + r[11] * pz;
    }
    __syncthreads();
    if (inside) {
      const float th = cam[12];
      const float u = (((float)x + 0.5f) / (float)a.W * 2.0f - 1.0f) * (th * (float)a.W / (float)a.H);
      const float w = (1.0f - ((float)y + 0.5f) / (float)a.H * 2.0f) * th;
      float wx = cam[9] + u * cam[3] + w * cam[6];
      float wy = cam[10] + u * cam[4] + w * cam[7];
      float wz = cam[11] + u * cam[5] + w * cam[8];
      const float inv = 1.0f / sqrtf(wx * wx + wy * wy + wz * wz);
      wx *= inv; wy *= inv; wz *= inv;
      float best = INFINITY, bnx = 0.0f, bny = 0.0f, bnz = 0.0f;   // nearest hit, its outward normal in the geom's frame
      int bg = -1;
      for (int g = 0; g < a.ngeom; g++) {
        const float* r = rec + g * REC;
        const float dx = r[3] * wx + r[6] * wy + r[9] * wz;
        const float dy = r[4] * wx + r[7] * wy + r[10] * wz;
        const float dz = r[5] * wx + r[8] * wy + r[11] * wz;
        const float ox = r[19], oy = r[20], oz = r[21];
        const float s0 = r[12], s1 = r[13], s2 = r[14];
        const int type = __float_as_int(r[15]);
        float t = INFINITY, nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (type == SUMO_GEOM_PLANE) {
          if (dz < 0.0f && oz > 0.0f) { t = -oz / dz; nz = 1.0f; }
        } else if (type == SUMO_GEOM_SPHERE) {
          float ts;
          if (sphere_entry(ox, oy, oz, dx, dy, dz, s0, &ts)) {
            t = ts; const float ir = 1.0f / s0;
            nx = (ox + t * dx) * ir; ny = (oy + t * dy) * ir; nz = (oz + t * dz) * ir;
          }
        } else if (type == SUMO_GEOM_CAPSULE || type == SUMO_GEOM_CYLINDER) {
          const float ir = 1.0f / s0;
          const float aa = dx * dx + dy * dy;
          if (aa > 1e-12f) {   // the wall: entry into the infinite cylinder, kept where it lies between the two ends
            const float t0 = -(ox * dx + oy * dy) / aa;
            const float px = ox + t0 * dx, py = oy + t0 * dy;
            const float disc = s0 * s0 - (px * px + py * py);
            if (disc >= 0.0f) {
              const float tw = t0 - sqrtf(disc / aa);
              if (fabsf(oz + tw * dz) <= s1) { t = tw; nx = (ox + tw * dx) * ir; ny = (oy + tw * dy) * ir; }
            }
          }
          for (int e = 0; e < 2; e++) {
            const float sg = e ? -1.0f : 1.0f, zc = oz - sg * s1;
            if (type == SUMO_GEOM_CAPSULE) {   // a hemisphere: the end sphere's entry where it lies beyond the end
              float ts;
              if (sphere_entry(ox, oy, zc, dx, dy, dz, s0, &ts) && (zc + ts * dz) * sg >= 0.0f && ts < t) {
                t = ts; nx = (ox + ts * dx) * ir; ny = (oy + ts * dy) * ir; nz = (zc + ts * dz) * ir;
              }
            } else if (dz * sg < 0.0f && zc * sg > 0.0f) {   // a flat end, seen from outside
              const float te = -zc / dz;
              const float px = ox + te * dx, py = oy + te * dy;
              if (px * px + py * py <= s0 * s0 && te < t) { t = te; nx = 0.0f; ny = 0.0f; nz = sg; }
            }
          }
        } else if (type == SUMO_GEOM_BOX) {   // slabs: the latest entry must precede the earliest exit
          const float o3[3] = {ox, oy, oz}, d3[3] = {dx, dy, dz}, h3[3] = {s0, s1, s2};
          float tn = -INFINITY, tf = INFINITY, sgn = 0.0f;
          int ax = -1;
          bool miss = false;
#pragma unroll
          for (int k = 0; k < 3; k++) {
            if (d3[k] == 0.0f) { miss = miss || fabsf(o3[k]) > h3[k]; continue; }
            const float id = 1.0f / d3[k], sd = d3[k] > 0.0f ? 1.0f : -1.0f;
            const float t1 = (-sd * h3[k] - o3[k]) * id, t2 = (sd * h3[k] - o3[k]) * id;
            if (t1 > tn) { tn = t1; ax = k; sgn = -sd; }
            tf = fminf(tf, t2);
          }
          if (!miss && ax >= 0 && tn < tf) {
            t = tn;
            nx = ax == 0 ? sgn : 0.0f; ny = ax == 1 ? sgn : 0.0f; nz = ax == 2 ? sgn : 0.0f;
          }
        }
        if (t > 0.0f && t + t * SUMO_RENDER_TIE_REL < best) { best = t; bg = g; bnx = nx; bny = ny; bnz = nz; }   // a tie keeps the lower id
      }
      const size_t pix = ((size_t)img * a.H + y) * a.W + x;
      if (a.depth) a.depth[pix] = best;
      if (a.id) a.id[pix] = bg;
      if (a.rgba) {
        float cr = a.shade.sky[0], cg = a.shade.sky[1], cb = a.shade.sky[2];
        if (bg >= 0) {
          const float* r = rec + bg * REC;
          const float gx = r[3] * bnx + r[4] * bny + r[5] * bnz;
          const float gy = r[6] * bnx + r[7] * bny + r[8] * bnz;
          const float gz = r[9] * bnx + r[10] * bny + r[11] * bnz;
          const float k = a.shade.ambient + a.shade.diffuse * fmaxf(0.0f, gx * lx_ + gy * ly_ + gz * lz_);
          cr = r[16] * k; cg = r[17] * k; cb = r[18] * k;
        }
        const uint32_t R8 = (uint32_t)rintf(255.0f * fminf(fmaxf(cr, 0.0f), 1.0f));
        const uint32_t G8 = (uint32_t)rintf(255.0f * fminf(fmaxf(cg, 0.0f), 1.0f));
        const uint32_t B8 = (uint32_t)rintf(255.0f * fminf(fmaxf(cb, 0.0f), 1.0f));
        a.rgba[pix] = R8 | (G8 << 8) | (B8 << 16) | 0xFF000000u;
      }
    }
    __syncthreads();   // the next image restages the records
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int sumo_render_create(const void* model_blob, size_t nbytes, int device, sumo_render_t* out) {
  if (!model_blob || !out) FAIL(-1, "bad arguments");
  sumo_render* h = new sumo_render();
  h->blob_dev = nullptr; h->gstat_dev = nullptr;
  h->blob.assign((const char*)model_blob, (const char*)model_blob + nbytes);
  int rc = sumo_model_parse(&h->hm, h->blob.data(), nbytes);
  if (rc != 0) { delete h; FAIL(-4, "malformed model blob (%d)", rc); }
  const sumo_model_t* m = &h->hm;
  if (m->ngeom < 1 || m->ngeom > MAXGEOM || m->nbody < 1 || m->nbody > MAXBODY) {
    const int ng = m->ngeom, nb = m->nbody;
    delete h;
    FAIL(-5, "scene with %d geoms / %d bodies is outside the renderer's capacity (%d geoms, %d bodies)", ng, nb, MAXGEOM, MAXBODY);
  }
  for (int b = 1; b < m->nbody; b++)   // the pose kernel reads parents before children and indexes its frames by these ids
    if (SUMO_I(m, body_parentid)[b] < 0 || SUMO_I(m, body_parentid)[b] >= b) { delete h; FAIL(-4, "malformed model blob (body order)"); }
  for (int g = 0; g < m->ngeom; g++)
    if (SUMO_I(m, geom_bodyid)[g] < 0 || SUMO_I(m, geom_bodyid)[g] >= m->nbody) { delete h; FAIL(-4, "malformed model blob (geom body)"); }
  for (int b = 0; b < m->nbody; b++) {
    const int ja = SUMO_I(m, body_jntadr)[b], jn = SUMO_I(m, body_jntnum)[b];
    if (jn < 0 || (jn > 0 && (ja < 0 || ja + jn > m->njnt))) { delete h; FAIL(-4, "malformed model blob (joint range)"); }
  }
  for (int j = 0; j < m->njnt; j++) {
    const int qa = SUMO_I(m, jnt_qposadr)[j], w = SUMO_I(m, jnt_type)[j] == SUMO_JNT_FREE ? 7 : 1;
    if (qa < 0 || qa + w > m->nq) { delete h; FAIL(-4, "malformed model blob (qpos address)"); }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { delete h; FAIL(-2, "no HIP device available: the renderer has no CPU fallback"); }
  if (device < 0 || device >= ndev) { delete h; FAIL(-3, "device %d out of range (%d devices)", device, ndev); }
  h->device = device;
  std::vector<float4> gstat(m->ngeom);
  for (int g = 0; g < m->ngeom; g++) {
    const double* s = SUMO_F(m, geom_size) + 3 * g;
    const int32_t type = SUMO_I(m, geom_type)[g];
    float tf;
    memcpy(&tf, &type, 4);
    gstat[g] = make_float4((float)s[0], (float)s[1], (float)s[2], tf);
  }
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc((void**)&h->blob_dev, nbytes);
  if (e == hipSuccess) e = hipMalloc((void**)&h->gstat_dev, sizeof(float4) * m->ngeom);
  if (e == hipSuccess) e = hipMemcpy(h->blob_dev, h->blob.data(), nbytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->gstat_dev, gstat.data(), sizeof(float4) * m->ngeom, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (h->blob_dev) (void)hipFree(h->blob_dev);
    if (h->gstat_dev) (void)hipFree(h->gstat_dev);
    delete h;
    FAIL(-100, "uploading the model failed: %s", hipGetErrorString(e));
  }
  h->dm = h->hm;
  h->dm.ibase = (const int32_t*)(h->blob_dev + ((const char*)h->hm.ibase - h->blob.data()));
  h->dm.fbase = (const double*)(h->blob_dev + ((const char*)h->hm.fbase - h->blob.data()));
  *out = h;
  return 0;
}

extern "C" int sumo_render_destroy(sumo_render_t h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  (void)hipFree(h->blob_dev);
  (void)hipFree(h->gstat_dev);
  delete h;
  return 0;
}

extern "C" int sumo_render_dims(sumo_render_t h, int32_t* out) {
  if (!h || !out) FAIL(-1, "bad arguments");
  out[0] = h->hm.nq; out[1] = h->hm.nbody; out[2] = h->hm.ngeom;
  return 0;
}

// 0 if p is device memory of `device`, else the failure is described in g_err
static int on_device(const void* p, int device, const char* what) {
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof at);
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    FAIL(-6, "%s is not device memory (device mismatch)", what);
  }
  if (at.type != hipMemoryTypeDevice || at.device != device)
    FAIL(-6, "%s is not memory of device %d (device mismatch)", what, device);
  return 0;
}
#define ONDEV(p, what) do { if (p) { int _r = on_device(p, h->device, what); if (_r) return _r; } } while (0)

extern "C" int sumo_render_poses(sumo_render_t h, const double* qpos_dev, int n, float* poses_dev, void* stream) {
  if (!h) FAIL(-1, "bad arguments");
  if (n < 1) FAIL(-1, "n must be >= 1 (got %d)", n);
  if (!qpos_dev || !poses_dev) FAIL(-1, "qpos and poses must not be NULL");
  ONDEV(qpos_dev, "qpos"); ONDEV(poses_dev, "poses");
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(render_poses_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->dm, qpos_dev, n, poses_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int sumo_render_frames(sumo_render_t h, const float* poses_dev, int n, const float* cams_dev, int ncam, const float* colors_dev,
                                  sumo_render_shade shade, int W, int H, uint8_t* rgba_dev, float* depth_dev, int32_t* id_dev, void* stream) {
  if (!h) FAIL(-1, "bad arguments");
  if (n < 1) FAIL(-1, "n must be >= 1 (got %d)", n);
  if (W < 1 || W > SUMO_RENDER_MAXDIM || H < 1 || H > SUMO_RENDER_MAXDIM)
    FAIL(-1, "width and height must lie in [1, %d] (got %d x %d)", SUMO_RENDER_MAXDIM, W, H);
  if (ncam != 1 && ncam != n) FAIL(-1, "ncam must be 1 or n = %d (got %d)", n, ncam);
  if (!poses_dev || !cams_dev || !colors_dev) FAIL(-1, "poses, cameras and colours must not be NULL");
  if (!rgba_dev && !depth_dev && !id_dev) FAIL(-1, "at least one of rgba, depth and id must be given");
  const double ll = sqrt((double)shade.light[0] * shade.light[0] + (double)shade.light[1] * shade.light[1] + (double)shade.light[2] * shade.light[2]);
  if (!(fabs(ll - 1.0) <= 1e-3)) FAIL(-1, "the light direction must have unit length (got %g)", ll);
  ONDEV(poses_dev, "poses"); ONDEV(cams_dev, "cameras"); ONDEV(colors_dev, "colours");
  ONDEV(rgba_dev, "rgba"); ONDEV(depth_dev, "depth"); ONDEV(id_dev, "id");
  HIPCHK(hipSetDevice(h->device));
  FrameArgs a;
  a.poses = poses_dev; a.cams = cams_dev; a.colors = colors_dev; a.gstat = h->gstat_dev;
  a.rgba = (uint32_t*)rgba_dev; a.depth = depth_dev; a.id = id_dev; a.shade = shade;
  a.n = n; a.ncam = ncam; a.ngeom = h->hm.ngeom; a.W = W; a.H = H; a.tiles_x = (W + TILE - 1) / TILE;
  const int tiles = a.tiles_x * ((H + TILE - 1) / TILE);
  hipLaunchKernelGGL(render_frames_kernel, dim3(tiles, n < 65535 ? n : 65535), dim3(TILE * TILE), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}
