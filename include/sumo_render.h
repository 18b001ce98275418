/* sumo_render.h -- C ABI of the match renderer (robosumo_selfplay_amd/csrc/sumo_render.hip -> libsumo_render.so).
 *
 * Two launches turn joint positions into pictures: sumo_render_poses (forward kinematics, float64, one thread per env) and
 * sumo_render_frames (an analytic ray caster: one thread per pixel, the env's geoms in LDS).  The library is independent of the
 * engine's (sumo_hip.h) and of the PPO library's (sumo_ppo.h): it reads the same model blob (sumo_model.h) and nothing else.
 *
 * Every function returns 0 or a negative code; sumo_render_last_error() describes the last failure of the calling thread.
 * `stream` is a hipStream_t passed as void* (NULL = the default stream).  All `_dev` pointers are device memory of the handle's
 * device.
 *
 * Conventions:
 *   - pixel (x, y), row 0 at the top; the ray goes through the pixel centre:
 *       d = normalize(forward + ((x + .5) / W * 2 - 1) * tanhalf * W / H * right + (1 - (y + .5) / H * 2) * tanhalf * up)
 *   - surfaces are seen from outside only (a plane from its +z side); the nearest hit with t > 0 wins, on a tie the lower geom
 *     id.  Two hits tie when they lie within SUMO_RENDER_TIE_REL of each other, relative: the scenes hold surfaces that coincide
 *     exactly (the concentric end hemispheres of two capsules that meet at a joint), and rounding must not pick the winner;
 *   - primitives as MuJoCo sizes them: plane = local z = 0, infinite; sphere radius size[0]; capsule / cylinder radius size[0],
 *     half length size[1] along local z (hemispherical caps / flat ends); box half sizes size[0..2];
 *   - channel = round(255 * clamp(base * (ambient + diffuse * max(0, n . light)), 0, 1)) with the outward normal n of the hit;
 *     no shadows, textures or anti-aliasing.
 */
#ifndef SUMO_RENDER_H
#define SUMO_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUMO_RENDER_MAXGEOM 128  /* geom records a block holds in LDS (96 B each); a scene with more geoms is refused at create */
#define SUMO_RENDER_MAXBODY 96   /* body frames a pose thread holds; a scene with more bodies is refused at create */
#define SUMO_RENDER_MAXDIM 4096  /* largest image width / height */
#define SUMO_RENDER_CAM_STRIDE 16 /* floats per camera record: eye, right, up, forward (an orthonormal basis), tan(fovy / 2), 3 x padding */
#define SUMO_RENDER_TIE_REL 1.9073486328125e-06f /* 2^-19: a later geom's hit replaces an earlier one's only if nearer by more than this, relative */
#define SUMO_RENDER_POSE_STRIDE 12 /* floats per geom pose: centre, then the 3x3 rotation (geom -> world) row-major */

typedef struct sumo_render* sumo_render_t;

/* shading constants, passed by value: the unit direction TOWARDS the light, the ambient and diffuse weights, the sky colour */
typedef struct sumo_render_shade {
  float light[3];
  float ambient;
  float diffuse;
  float sky[3];
} sumo_render_shade;

const char* sumo_render_last_error(void);

/* Parses the blob (sumo_model_parse), refuses ngeom > SUMO_RENDER_MAXGEOM and nbody > SUMO_RENDER_MAXBODY, uploads the kinematic
 * tables and the geom tables (type, size, local pos and quat, body id) to `device`. */
int sumo_render_create(const void* model_blob, size_t nbytes, int device, sumo_render_t* out);
int sumo_render_destroy(sumo_render_t h);

/* out[0..2] = nq, nbody, ngeom */
int sumo_render_dims(sumo_render_t h, int32_t* out);

/* Geom poses of n envs: qpos_dev float64 [n][nq] -> poses_dev float32 [n][ngeom][12].  Forward kinematics in float64, rounded once
 * on store: a free joint takes its position and its normalised quaternion from qpos, hinges rotate about jnt_axis by
 * qpos - qpos0 about the joint anchor, bodies in id order. */
int sumo_render_poses(sumo_render_t h, const double* qpos_dev, int n, float* poses_dev, void* stream);

/* n images of W x H pixels from n pose sets.  cams_dev float32 [ncam][16] with ncam == n (one camera per image) or 1 (shared);
 * colors_dev float32 [ngeom][3].  Outputs, any of which may be NULL (not all three): rgba_dev uint8 [n][H][W][4] (alpha 255),
 * depth_dev float32 [n][H][W] (distance along the unit ray, +inf for sky), id_dev int32 [n][H][W] (geom hit, -1 for sky).
 * Refused before any launch: n < 1, W or H outside [1, SUMO_RENDER_MAXDIM], ncam other than 1 or n, poses / cams / colours NULL,
 * all outputs NULL, a light direction that is not unit length to 1e-3, a pointer that is not memory of the handle's device. */
int sumo_render_frames(sumo_render_t h, const float* poses_dev, int n, const float* cams_dev, int ncam, const float* colors_dev,
                       sumo_render_shade shade, int W, int H, uint8_t* rgba_dev, float* depth_dev, int32_t* id_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUMO_RENDER_H */
