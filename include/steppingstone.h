/*
 * steppingstone.h -- C ABI of libsteppingstone.so: the MI355X-native vectorised stepping-stone environment.
 *
 * The reference has no FFI for this path: its boundary is the Python object protocol between
 * common/envs_utils.py (ShmemVecEnv / _subproc_worker) and the gym env in the un-vendored mocca_envs submodule.
 * Every entry point below therefore cites the reference call site(s) whose job it takes over.  A reference
 * maintainer binds these with ctypes (INTEGRATION.md shows the stub); no torch types cross this boundary.
 *
 * Conventions: all functions return 0 on success or a negative ss_status; ss_last_error() returns a thread-local
 * message.  The caller owns every I/O buffer (device pointers, e.g. tensor.data_ptr()); the library owns the
 * structure-of-arrays environment state in HBM.  Every entry point that takes a stream (hipStream_t as void*;
 * NULL = the null stream) only enqueues work on it and never synchronises the host.  The hooks WITHOUT a stream
 * argument (ss_set_curriculum / _specialist / _sample_prob / _power / _auto_reset) are host-synchronous: they
 * copy <= 500 bytes (the [N,11,11] per-env grid of ss_set_sample_prob: N x 484 B) to the device-resident hook
 * state before returning, so every step enqueued afterwards -- on any stream, or replayed from a captured
 * hipGraph -- sees the new value; a step still in flight when a hook is called may see either (as in the
 * reference, hooks belong between step_wait() and the next step_async()).  ss_set_sample_prob_device is the
 * stream-ordered, sync-free form for grids that are computed on the GPU.  One handle per (process, device); a
 * handle is not thread-safe.
 */
#ifndef STEPPINGSTONE_H
#define STEPPINGSTONE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS_OBS_DIM 60     /* shipped checkpoints: actor.state_dim */
#define SS_ACT_DIM 21     /* common/render_utils.py:47-69 */
#define SS_GRID 11        /* playground/train.py:132-133 (11x11 yaw x pitch grid, centre index 5) */
#define SS_NCELL 121
#define SS_NUM_STONES 20
#define SS_STATE_DIM 186  /* packed per-env state of ss_get_state / ss_set_state */
#define SS_INFO_WORDS 6    /* 32-bit words of ss_info */
#define SS_ABI_VERSION 4   /* ss_version(): 2 -> 3 added ss_info.ep_ret_lo and state word 185 (round 3); 3 -> 4 (round 4) changed a
                            * MEANING, no layout: actions and observations carry POLICY coordinates, see "Joint conventions".
                            * The rendering entry points (ss_camera, ss_camera_default, ss_body_poses, ss_render) and the per-env
                            * episode control (ss_reset_masked, ss_get_state_envs, ss_set_state_envs) were ADDED under version 4: no
                            * existing layout or meaning changed, so a version-4 binding keeps working.  So was the kinematic
                            * readout (ss_kinematics), the force readout (ss_step_forces) and the equation-of-motion readout
                            * (ss_eom), the impulse (ss_push), the one addition that writes: velocities only, and the look-ahead
                            * (ss_lookahead), which writes nothing of an env, with its from-states form (ss_lookahead_states) and
                            * the observation of state rows (ss_get_obs_states). */
#define SS_MAX_EPISODE_STEPS 1000

typedef enum { SS_WALKER3D = 0, SS_MIKE = 1 } ss_kind;   /* ids: README.md:27,31 of the reference */

typedef enum {
  SS_OK = 0,
  SS_ERR_INVALID = -1,   /* bad argument */
  SS_ERR_HIP = -2,       /* a HIP runtime call failed (message has hipGetErrorString) */
  SS_ERR_NO_DEVICE = -3, /* no gfx950 device visible: there is NO CPU fallback */
  SS_ERR_ALLOC = -4
} ss_status;

/* per-env step report; replaces the `info` dict built by Monitor.update (common/envs_utils.py:131-153) and
 * TimeLimitMask.step (:59-65) plus env.update_terrain (playground/train.py:245). ep_* valid when done. */
typedef struct {
  float ep_ret;            /* info["episode"]["r"], leading part (the fp32 nearest to the episode return) */
  float ep_len;            /* info["episode"]["l"] */
  int32_t bad_transition;  /* info["bad_transition"] */
  int32_t steps_reached;   /* next_step_index at the end of the step */
  int32_t update_terrain;  /* env.update_terrain */
  /* Monitor.update sums the step rewards as Python floats and reports round(sum, 6) (common/envs_utils.py:131-138).  The
   * kernel keeps the running sum as an unevaluated pair of floats (error-free two-sum per step):
   * (double)ep_ret + (double)ep_ret_lo is the fp64 sum of the fp32 step rewards to ~1e-11; the host rounds it to 6 decimals. */
  float ep_ret_lo;
} ss_info;

typedef struct ss_env ss_env;

/* gym.make(env_id) + env.seed(seed + rank) for num_envs envs at once (common/envs_utils.py:25-40,48-56).
 * env_id_offset: global index of this handle's first env (multi-GPU sharding keeps RNG streams rank-invariant). */
int ss_create(ss_env** out, int kind, int32_t num_envs, int device, uint64_t seed, int64_t env_id_offset);
void ss_destroy(ss_env* env);                                   /* env.close(), envs_utils.py:667-676 */
const char* ss_last_error(void);

/* Joint conventions.  Joint / action order: common/render_utils.py:47-69 (abdomen z,y,x; right hip x,z,y, knee, ankle; left ...;
 * right shoulder x,z,y, elbow; left ...).  POLICY coordinates -- act[j], obs[6+j] (normalised angle), obs[27+j] (0.1 * rate):
 * sigma_j x (value about the +axis of the link frame), docs/PHYSICS.md 2, sigma = model.POLICY_SIGN: -1 for the left limbs' x / z
 * joints (measured about the MIRRORED axis, so that ss_get_mirror_indices swaps the limbs without negating them) and for both knees
 * (negative in flexion), +1 elsewhere: the conventions the reference's shipped actors were trained in (playground/models/ *.pt are
 * mirror-equivariant under exactly these lists and reject the other knee sign, tests/test_shipped_policy_layout.py).
 * ss_get_state / ss_set_state keep every angle about the +axis.
 *
 * ShmemVecEnv.reset (envs_utils.py:542-548): obs [num_envs, 60] f32 row-major, device pointer. */
int ss_reset(ss_env* env, float* obs, void* stream);

/* ShmemVecEnv.step_async + step_wait + worker auto-reset (envs_utils.py:550-558, 646-649).
 * act [N,21] f32; obs [N,60] f32; rew [N] f32; done [N] u8; info [N] ss_info (may be NULL).  Device pointers. */
int ss_step(ss_env* env, const float* act, float* obs, float* rew, uint8_t* done, ss_info* info, void* stream);

/* Benchmark path (BASELINE.json metric "batched random-action rollout"): num_steps control steps with
 * on-device Philox actions U(-1,1); t0 = index of the first step in the action stream.  steps_per_launch control
 * steps run inside ONE kernel launch with the state resident in LDS between them (0 = default 1000; 1 = one launch
 * per step, the ss_step code path).  Every step writes obs / rew / done / info (the buffers hold the last step's
 * values afterwards) and the HBM copy of the state; the result is bit-identical for every steps_per_launch. */
int ss_rollout_random(ss_env* env, int32_t num_steps, int32_t steps_per_launch, uint64_t t0, float* obs, float* rew,
                      uint8_t* done, ss_info* info, void* stream);
/* The same multi-step launch writing every step's packed block (see ss_step_packed) at packed[k] of a [num_steps, N, 62]
 * f32 device buffer: the rollout of a multi-GPU shard whose exchange ships num_steps blocks per collective instead of one
 * (steppingstone_amd.distributed.ShardedVecEnv.rollout_random: same bytes on the wire, K times fewer collectives and
 * launches).  One launch; num_steps >= 1. */
int ss_rollout_random_packed(ss_env* env, int32_t num_steps, uint64_t t0, float* packed, ss_info* info, void* stream);
/* One step whose results land in ONE packed device buffer [N,62] f32 = obs(60) | rew | done(0/1): the block a
 * multi-GPU shard all-gathers per step (replaces the per-env pipe + shared-memory traffic of
 * common/envs_utils.py:550-558,608-620).  use_random_actions != 0: actions from the benchmark Philox stream at index t. */
int ss_step_packed(ss_env* env, const float* act, int use_random_actions, uint64_t t, float* packed, ss_info* info,
                   void* stream);
/* Peer-store all-gather: the multi-GPU exchange of SURVEY.md 8e WITHOUT a collective in the data path.  Every rank owns
 * a gather buffer [G * N_local, 62] f32 and a flag array [G] u32 in fine-grained device memory (ss_peer_alloc; shared
 * with the other ranks' processes through ss_peer_ipc_handle / ss_peer_ipc_open, 64-byte handles), one pair per ring
 * slot.  ss_peer_connect gives the handle the gather-buffer and flag-array pointers of all G ranks as seen from THIS
 * process (index = slot * G + rank; own entries included).
 * ss_step_packed_peers is ss_step_packed whose kernel additionally stores its rows straight into every peer's gather
 * buffer (xGMI peer-to-peer stores) and, from the last workgroup, publishes step_id in flag[rank] of every peer.
 * ss_peer_wait enqueues a one-wavefront kernel that returns once all G peers have published step_id (or later) here:
 * work enqueued behind it may read this rank's gather buffer.  step_id must increase from launch to launch; a buffer
 * may be overwritten only after every peer has consumed it (use >= 2 buffers in turn).  ss_peer_error: non-zero if a
 * wait timed out.  (packed may be NULL here: the gather buffer already holds this rank's own rows.) */
int ss_peer_alloc(void** out, uint64_t bytes);
int ss_peer_free(void* ptr);
int ss_peer_ipc_handle(void* ptr, void* handle64);
int ss_peer_ipc_open(const void* handle64, void** out);
int ss_peer_ipc_close(void* ptr);
int ss_peer_connect(ss_env* env, int32_t count, int32_t rank, int32_t slots, float* const* gather_bufs,
                    uint32_t* const* flag_bufs);          /* pointer tables [slots][count]; slots <= 4 buffers used in turn */
int ss_step_packed_peers(ss_env* env, const float* act, int use_random_actions, uint64_t t, int32_t slot, uint32_t step_id,
                         float* packed, ss_info* info, void* stream);
int ss_peer_wait(ss_env* env, int32_t slot, uint32_t step_id, void* stream);
int ss_peer_error(ss_env* env, uint32_t* out);
/* Same action stream written to act [N,21] (parity tests / external policies). */
int ss_random_actions(ss_env* env, uint64_t t, float* act, void* stream);

/* Curriculum hooks (envs_utils.py:568-590, 650-664; playground/train.py:118,122,271). */
int ss_set_curriculum(ss_env* env, int32_t level);              /* env.update_curriculum */
int ss_set_specialist(ss_env* env, int32_t level);              /* env.update_specialist */
/* env.update_sample_prob: HOST pointer to f64 probabilities, [N,11,11] if per_env else [11,11]. */
int ss_set_sample_prob(ss_env* env, const double* prob, int per_env);
/* Same hook for a grid that already lives on the GPU (the batched threshold / adaptive sampler computes it there,
 * playground/train.py:229-272): DEVICE pointer to f32 probabilities, [N,11,11] if per_env else [11,11]; the copy /
 * transpose and the switch to the new grid are ordered on `stream`, the host is not synchronised (the first per-env
 * call allocates the [121][N] table). */
int ss_set_sample_prob_device(ss_env* env, const float* prob, int per_env, void* stream);
/* env.set_mirror (common/envs_utils.py:588-590, train.py:109-111).  Accepted for protocol compatibility ONLY -- it stores
 * nothing and changes nothing: the Walker3D / Mike observation has no gait-phase term for the flag to act on (the reference
 * uses it with phase-clocked envs); the symmetry a learner needs is ss_get_mirror_indices. */
int ss_set_mirror(ss_env* env, int32_t on);
int ss_set_power(ss_env* env, float power);                     /* env.set_robot_params({"power": p}) */
/* on (default): worker semantics, a finished env is reset inside the step (envs_utils.py:647-648);
 * off: plain gym env semantics for make_env() users -- terminal obs returned, caller resets (train.py:243-244); a batch resets its
 * finished envs with ss_reset_masked. */
int ss_set_auto_reset(ss_env* env, int32_t on);

/* env.create_temp_states (train.py:247, envs_utils.py:573-578): out [N,121,60] f32, device pointer. */
int ss_create_temp_states(ss_env* env, float* out, void* stream);

/* env.unwrapped.get_mirror_indices() (train.py:160; consumed by get_mirror_function, envs_utils.py:687-694).
 * buf receives the 6 index lists back to back, lens[6] their lengths; buf must hold 2*(60+21) int32.
 * Lists (policy coordinates): negated obs {vy, roll, abdomen z / x angle and rate, sin(dtheta) d and x_tilt of both targets},
 * negated act {abdomen z, x}; right <-> left: the 9 limb joints (angle, rate, action) and the two contact flags. */
int ss_get_mirror_indices(int kind, int32_t* buf, int32_t* lens);

/* Full-state injection / extraction for parity tests and terrain_info (enjoy.py:60-64).  DEVICE pointers,
 * [N, SS_STATE_DIM] f32 row-major:
 *   0:3 pos | 3:7 quat wxyz | 7:13 base twist (body frame, angular first) | 13:34 q | 34:55 qd |
 *   55 pot_prev | 56 z_init | 57 ep_ret | 58 next-next dr | 59 next_step_index | 60 target_reached_count |
 *   61 elapsed | 62 rng_ctr & 0xffff | 63 rng_ctr >> 16 | 64 flags (bit0 right, bit1 left foot contact) |
 *   65:185 terrain_info [20][6] = x,y,z,phi,x_tilt,y_tilt | 185 ep_ret_lo (trailing part of the episode return) */
int ss_get_state(ss_env* env, float* packed, void* stream);
int ss_set_state(ss_env* env, const float* packed, void* stream);
/* Observation of the current state without stepping (used after ss_set_state). */
int ss_get_obs(ss_env* env, float* obs, void* stream);

/* Per-env episode control: the reference resets each env in its own worker process (common/envs_utils.py:642-649); these reset or
 * move a subset of the batch.  Added under version 4 (no existing layout or meaning changed).  All three are ordered on `stream`,
 * never synchronise the host, allocate nothing and can be captured into a hipGraph.  Bad host-side arguments return SS_ERR_INVALID
 * and launch nothing.
 *
 * ss_reset_masked: resets env e iff mask[e] != 0 (mask: DEVICE [N] u8; the done output of ss_step is a valid mask), the reset of
 * ss_reset.  obs (may be NULL: state only) receives the fresh observation in row e, with a row stride of obs_stride floats: 60 for
 * ss_step's [N,60] obs, 62 for ss_step_packed's [N,62] block (its rew / done words are left alone).  terminal_obs (optional, DEVICE
 * [N,60], needs obs): row e receives row e of obs as it was BEFORE the reset, i.e. the terminal observation of a finished step.
 * An env with mask[e] == 0 is not touched: no state word, obs row or terminal row is read or written.  With auto-reset off, ss_step
 * followed by ss_reset_masked(done) leaves exactly the state, obs, rew, done and info of ss_step with auto-reset on.
 * obs_stride must be 60 or 62.
 *
 * ss_get_state_envs / ss_set_state_envs: ss_get_state / ss_set_state for the m envs listed in env_ids (DEVICE [m] int32): row k of
 * packed ([m, SS_STATE_DIM] f32, the layout above) <-> env env_ids[k].  m >= 0 (0: nothing happens); env_ids and packed may be NULL
 * only when m == 0.  An id outside [0, N) lives on the device and is not checked here: it is skipped (no row read or written).
 * Duplicate ids in ss_set_state_envs: which row lands in that env is unspecified (the words may even mix rows); callers pass
 * distinct ids. */
int ss_reset_masked(ss_env* env, const uint8_t* mask, float* obs, int32_t obs_stride, float* terminal_obs, void* stream);
int ss_get_state_envs(ss_env* env, const int32_t* env_ids, int32_t m, float* packed, void* stream);
int ss_set_state_envs(ss_env* env, const int32_t* env_ids, int32_t m, const float* packed, void* stream);

int32_t ss_num_envs(const ss_env* env);
/* SS_ABI_VERSION of the library.  A binding must check it at load time (steppingstone_amd/_lib.py does): version 2 inserted
 * steps_per_launch into ss_rollout_random's argument list, version 3 grew ss_info to 6 words and the packed state to 186,
 * version 4 changed the sign convention of the left limbs' x / z joints and of the knees in actions and observations (same layouts). */
int ss_version(void);

/* Rendering (docs/RENDER.md is the specification).  Both calls only READ the environment state, are ordered on `stream`, never
 * synchronise the host and allocate nothing: they can be captured into a hipGraph next to the steps.
 * ss_camera: mode SS_CAM_TRACK (default) -- target = torso position + target[], eye = target + eye[] (world-frame offsets);
 * SS_CAM_CHASE -- the same with both offsets turned by the torso's yaw (per-env pixel observations); SS_CAM_FIXED -- eye[] and
 * target[] in world coordinates.  Vertical field of view fov_y_deg in (0, 180); far_m > 0 (depth of the background, and no hit at or
 * beyond it counts); flags bit 0: hard shadows.  eye[] and target[] must be finite and the view vector (eye[] for TRACK / CHASE,
 * target[] - eye[] for FIXED) at least 1e-6 m long: a camera without a view direction is refused.  ss_camera_default fills the TRACK camera that frames a reset robot and its next stone. */
typedef enum { SS_CAM_TRACK = 0, SS_CAM_CHASE = 1, SS_CAM_FIXED = 2 } ss_camera_mode;
#define SS_CAM_SHADOWS 1
typedef struct {
  int32_t mode;
  float eye[3];
  float target[3];
  float fov_y_deg;
  float far_m;
  int32_t flags;
} ss_camera;
int ss_camera_default(ss_camera* cam);
/* World pose of all 22 bodies (torso = body 0, body j+1 = child link of joint j): out [N, 22, 12] f32 = position | R row-major,
 * the frame convention of steppingstone_amd/model.py fk().  DEVICE pointer, 16-byte aligned. */
int ss_body_poses(ss_env* env, float* out, void* stream);
/* Frames of the m envs listed in env_ids (DEVICE [m] int32): rgb [m,H,W,3] u8, depth [m,H,W] f32 (z-depth; background = far_m),
 * seg [m,H,W] u8 (0 background, 1 + body, 23 / 24 / 25 the stones n-1 / n / n+1).  Any output may be NULL, not all three; rgb and seg
 * must be 4-byte aligned.  width and height: multiples of 4 in 4..2048; m >= 1.  Bad arguments return SS_ERR_INVALID and launch
 * nothing.  An env id outside [0, N) lives on the device and is not checked here: that env is drawn as background. */
int ss_render(ss_env* env, const int32_t* env_ids, int32_t m, int32_t width, int32_t height, const ss_camera* cam, uint8_t* rgb,
              float* depth, uint8_t* seg, void* stream);

/* Whole-body kinematic readout of the m envs listed in env_ids (docs/PHYSICS.md "Kinematic readout" has the definitions); added under
 * version 4 (nothing existing moved).  It only READS the environment state, is ordered on `stream`, never synchronises the host and
 * allocates nothing.  env_ids: DEVICE [m] int32 as in ss_get_state_envs, row k of every output describes env env_ids[k]; env_ids ==
 * NULL means envs 0..m-1 and needs m == N.  m == 0 does nothing.  An id outside [0, N) lives on the device and is not checked here: no
 * row of it is read or written.  Outputs are DEVICE pointers, 16-byte aligned, f32; any may be NULL, not all three when m > 0.  Bad host
 * arguments return SS_ERR_INVALID and launch nothing.  A row's bits depend on the env's state alone: not on N, m, k or the outputs asked for.
 *   body_twist [m,22,6]: world-frame twist of body b (the bodies and link frames of ss_body_poses; massless intermediate links
 *     included): 0:3 angular velocity, 3:6 linear velocity of the origin of the link frame.
 *   summary [m,SS_KIN_SUMMARY]: 0:3 centre of mass | 3:6 its velocity (total linear momentum / total mass) | 6:9 angular momentum about
 *     the centre of mass | 9 kinetic energy of the rigid bodies, sum_b (m_b |v_c,b|^2 + w_b . I_c,b w_b) / 2 -- the rotor ARMATURE of
 *     the joints (PHYSICS.md 3.1) is NOT included | 10 potential energy M * 9.8 * com_z | 11 total mass M.
 *   corners [m,SS_KIN_CORNER,8]: sole corner c = 4 * foot + corner (foot 0 = right, 1 = left; corner order of the model's `corners`,
 *     PHYSICS.md 2): 0:3 world position | 3:6 world velocity | 6 signed height h = (x - s_n) . n_n over the surface plane of the
 *     target stone n (negative below the surface; the contact set is -0.10 < h < 0) | 7 carrier, as a float: 0, 1 or 2 when the stone
 *     in slot n-1, n or n+1 carries the corner (PHYSICS.md 3.3: the decision of the step kernels' own detection code, tie rule
 *     included), -1 when none does. */
#define SS_KIN_SUMMARY 12
#define SS_KIN_CORNER 8
int ss_kinematics(ss_env* env, const int32_t* env_ids, int32_t m, float* body_twist, float* summary, float* corners, void* stream);

/* Force readout: a DRY RUN of one control step of the m envs listed in env_ids under the actions act (docs/PHYSICS.md "Force readout"
 * has the definitions); added under version 4 (nothing existing moved).  It runs the four substeps of ss_step on a copy of the state
 * and reports what they do; it only READS the environment state (no state word, terrain row or RNG counter changes), is ordered on
 * `stream`, never synchronises the host and allocates nothing.  No reward, termination, target logic or reset is evaluated.
 * env_ids: DEVICE [m] int32 with the conventions of ss_kinematics (NULL: envs 0..m-1, needs m == N; m == 0 does nothing; an id outside
 * [0, N) is skipped: no row of it is read or written).  act: DEVICE [m, 21], row k is the action for env env_ids[k], policy coordinates,
 * clipped as in ss_step.  Outputs are DEVICE pointers, 16-byte aligned, f32; any may be NULL, not all three when m > 0.  Bad host
 * arguments return SS_ERR_INVALID and launch nothing.  A row's bits depend on the env's state, the knobs (ss_set_power) and its action
 * row alone: not on N, m, k, repeated ids or the outputs asked for.
 *   contacts [m, SS_FRC_SUBSTEPS, 8, SS_FRC_CONTACT]: substep s, sole corner c = 4 * foot + corner (the order of ss_kinematics):
 *     0 carrier slot as a float (0, 1, 2: stone n-1, n, n+1; -1: none; the coding of ss_kinematics corners word 7), the detection at
 *     the START of substep s | 1 penetration in metres | 2:5 contact force over the substep, lambda / h along n, t1, t2 of PHYSICS.md
 *     3.4, in newtons | 5:8 the same force as a world vector.  A corner that is not carried has words 1:8 exactly 0.
 *   joints [m, SS_FRC_SUBSTEPS, SS_FRC_JOINT, 21], joint order and +axis convention of ss_get_state: row 0 q, row 1 qd at the start
 *     of substep s | row 2 the explicit torque tau_j of PHYSICS.md 3.1 | row 3 the torque the joint applied over the substep under the
 *     linearly-implicit scheme, tau_j - (Dadd_j - armature_j) (qd+_j - qd_j) / h.
 *   next_state [m, SS_FRC_STATE]: words 0:55 of the ss_get_state layout after the four substeps | 55 flags as a float: bit 0 / 1 right /
 *     left foot contact, bit 2 / 3 right / left foot touches the target stone, both of the last substep's detection. */
#define SS_FRC_SUBSTEPS 4
#define SS_FRC_CONTACT 8   /* words per corner row */
#define SS_FRC_JOINT 4     /* rows per substep */
#define SS_FRC_STATE 56
int ss_step_forces(ss_env* env, const int32_t* env_ids, int32_t m, const float* act,
                   float* contacts, float* joints, float* next_state, void* stream);

/* Equation-of-motion readout of the m envs listed in env_ids (docs/PHYSICS.md "Equation of motion readout" has the definitions); added
 * under version 4 (nothing existing moved).  It only READS the environment state, is ordered on `stream`, never synchronises the host
 * and allocates nothing.  env_ids: DEVICE [m] int32 with the conventions of ss_kinematics (NULL: envs 0..m-1, needs m == N; m == 0 does
 * nothing; an id outside [0, N) is skipped: no row of it is read or written).  Outputs are DEVICE pointers, 16-byte aligned, f32; any
 * may be NULL, not all three when m > 0.  Bad host arguments return SS_ERR_INVALID and launch nothing.  A row's bits depend on the env's
 * state alone: not on N, m, k, repeated ids or the outputs asked for.
 * Generalised velocity nu = [w_b (3); v_b (3); qd (21)] = state words 7:13 | 34:55: the base twist in body coordinates, the joints in the
 * order and about the +axis of ss_get_state.  DoF i < 6 is the base, DoF 6 + j is joint j.
 *   mass [m, SS_EOM_DOF, SS_EOM_DOF]: joint-space inertia M(q) = H(q) + diag(0_6, armature): the composite-rigid-body matrix of the 22
 *     bodies plus the rotor armature of PHYSICS.md 3.1 on the joint diagonal.  Both triangles are written, M == M^T bit for bit.
 *   forces [m, SS_EOM_FORCES, SS_EOM_DOF]: row 0 c(q, nu), the velocity-product (Coriolis / centrifugal) generalised force: inverse
 *     dynamics at zero acceleration without gravity, base rows included | row 1 g(q) = M[:, 3:6] R^T (0, 0, -9.8), the generalised
 *     force of gravity | row 2 passive: [0_6; -damping qd - stiffness q - kl viol - dl qd], the joints' springs, dampers and limits in
 *     continuous time (PHYSICS.md 3.1's tau_j at h = 0 and tau_m = 0).
 *   corner_jac [m, SS_KIN_CORNER, 3, SS_EOM_DOF]: J_c with x_c-dot = J_c nu the world velocity of sole corner c = 4 * foot + corner (the
 *     order of ss_kinematics), carried or not.
 * Together: M nu-dot + c = g + [0; tau_m + passive] + sum_c J_c^T f_c, f_c the world contact force on corner c. */
#define SS_EOM_DOF 27      /* 6 base + 21 joints */
#define SS_EOM_FORCES 3    /* rows of `forces` */
int ss_eom(ss_env* env, const int32_t* env_ids, int32_t m, float* mass, float* forces, float* corner_jac, void* stream);

/* Impulse: push body body[k] of env env_ids[k] (docs/PHYSICS.md "Impulse" has the definitions); added under version 4 (nothing existing
 * moved).  delta_nu = M(q)^-1 J^T w: M the `mass` of ss_eom (rotor armature included), nu its generalised velocity (state words 7:13 |
 * 34:55), J the 6 x 27 Jacobian of the pushed point ([x-dot; omega_b] = J nu, world axes), w the wrench impulse.  Contacts, joint limits
 * and the implicit damping of PHYSICS.md 3.1 do not enter: the push is instantaneous, positions do not move, and the next substep's
 * detection and contact solve see the new velocities.  Total linear momentum changes by exactly p, angular momentum about the centre of
 * mass by (x - com) x p + L.  Ordered on `stream`, never synchronises the host, allocates nothing, can be captured into a graph.
 *   env_ids: DEVICE [m] int32 with the conventions of ss_eom (NULL: envs 0..m-1, needs m == N; m == 0 does nothing; an id outside [0, N)
 *     is skipped: nothing of it is read or written).
 *   body: DEVICE [m] int32 in [0, 22), the bodies of ss_body_poses; NULL: the torso for every row.  An index outside the range lives on
 *     the device and is not checked here: that row is skipped like a bad id.
 *   point: DEVICE [m,3] f32, the pushed point in the body's link frame; NULL: the body's centre of mass (the link origin of a massless
 *     intermediate link).
 *   impulse: DEVICE [m, SS_PUSH_WRENCH] f32, world axes: 0:3 linear impulse p in N s acting at the point | 3:6 pure angular impulse L in
 *     N m s.  Required when m > 0.
 *   delta_nu: DEVICE [m, SS_EOM_DOF] f32, 16-byte aligned, or NULL: receives delta_nu.
 *   apply != 0: state words 7:13 and 34:55 of env env_ids[k] become nu + delta_nu; no other word, no other env and no RNG counter
 *     changes.  With repeated ids the result for that env is unspecified, as in ss_set_state_envs; the effect is linear, so two pushes on
 *     one env are two dry runs added.  apply == 0: a dry run, which needs delta_nu.
 * Bad host arguments return SS_ERR_INVALID and launch nothing.  A row's delta_nu bits depend on the env's state and on that row's body,
 * point and impulse alone: not on N, m, k, apply or on delta_nu being asked for.  An all-zero impulse row yields delta_nu exactly 0. */
#define SS_PUSH_WRENCH 6   /* words of an impulse row */
int ss_push(ss_env* env, const int32_t* env_ids, int32_t m, const int32_t* body, const float* point, const float* impulse,
            float* delta_nu, int32_t apply, void* stream);

/* Look-ahead: dry-run `horizon` control steps of ss_step for action sequences (docs/PHYSICS.md "Look-ahead" has the definitions); added
 * under version 4 (nothing existing moved).  Row k is a BRANCH of env env_ids[k]: horizon control steps from that env's current state
 * under the action rows act[k, 0..horizon-1, :], on a private copy of everything a step reads or writes (dynamic state, active stones and
 * headings, the terrain row, target counters, episode statistics, the RNG counter).  NOTHING of the env changes: no state word, no terrain
 * row, no RNG counter, no knob.  A branch sees what the env itself would see: its target advances, and the stones drawn on an advance,
 * come from the env's own counter, global id, curriculum and probability grid; ss_set_power applies; the auto-reset switch is ignored (a
 * branch never resets).  Ordered on `stream`, never synchronises the host, allocates nothing, can be captured into a graph.
 *   env_ids: DEVICE [m] int32 with the conventions of ss_step_forces (NULL: envs 0..m-1, needs m == N; m == 0 does nothing; an id outside
 *     [0, N) is skipped: nothing of it is read, no output row of it is written).  Repeated ids are the normal use: B branches of one env
 *     are B rows with its id.
 *   horizon: 1 .. SS_LOOK_MAX_STEPS.
 *   act: DEVICE [m, horizon, 21] f32, policy coordinates, clipped as in ss_step (a NaN ends the episode as there).
 *   obs: DEVICE [m, horizon, 60] f32 or NULL; rew: DEVICE [m, horizon] f32; done: DEVICE [m, horizon] u8: for every step s up to and
 *     including the first with done, bit for bit what ss_step writes for that env with auto-reset off, stepped s + 1 times under the same
 *     actions (the time limit counts).  Every later step of the row: done = 1, rew = 0.0f, the observation repeats the terminal row.
 *   final_state: DEVICE [m, SS_STATE_DIM] f32 or NULL: bit for bit ss_get_state_envs of the env after those real steps -- the state the
 *     finishing step ended in, or the state after step horizon - 1.
 *   work: DEVICE [m, SS_LOOK_WORK] f32, required when m > 0: where a branch keeps its private copy; its contents afterwards are
 *     unspecified.
 *   obs, rew, final_state and work are 16-byte aligned.
 * Bad host arguments return SS_ERR_INVALID and launch nothing.  A row's bits depend on the env's state, the knobs and that row's actions
 * alone: not on N, m, k, repeated ids, on which outputs were asked for, or on the steps behind them (the first H' steps of a call with
 * horizon > H' are those of a call with horizon H'). */
#define SS_LOOK_MAX_STEPS 1000          /* = SS_MAX_EPISODE_STEPS */
#define SS_LOOK_WORK 160                /* f32 words of workspace per row */
int ss_lookahead(ss_env* env, const int32_t* env_ids, int32_t m, int32_t horizon, const float* act,
                 float* obs, float* rew, uint8_t* done, float* final_state, float* work, void* stream);

/* Look-ahead from caller-supplied states (docs/PHYSICS.md "Branches from caller-supplied states"); added under version 4 (nothing
 * existing moved).  Row k is a branch of env env_ids[k] that starts from states[k, :] instead of that env's current state: its obs, rew,
 * done and final_state rows are bit for bit what ss_lookahead writes for a row with that id and those actions after ss_set_state_envs
 * has put states[k] into env env_ids[k].  NOTHING of the env changes: no state word, no terrain row, no RNG counter, no knob.  The env
 * supplies what a state row does not carry: its global id (the Philox key of the stones drawn on an advance), its row of a per-env
 * probability grid, the curriculum level, the shared grid and ss_set_power.  The RNG counter is the row's (words 62 and 63).  The row is
 * read as ss_set_state reads it: the integer words through (int), all 20 terrain rows as stored, the active stones' normals and headings
 * from the terrain words of stones n-1, n, n+1 (n = word 59; the three indices are clamped into [0, 19], which changes nothing for a
 * state ss_step accepts, 1 <= n <= 19: no row, whatever its 186 words hold, makes the call read or write outside that row's own
 * buffers), the quaternion as given.
 *   states: DEVICE [m, SS_STATE_DIM] f32, the ss_get_state layout, required when m > 0; 4-byte aligned (final_state + k * SS_STATE_DIM of
 *     an earlier call can be passed as it is).  Only read.
 *   env_ids, horizon, act, obs, rew, done, final_state, work: as in ss_lookahead, word for word -- frozen rows behind a first done, the
 *     time limit, a NaN action, repeated ids (now each with its own state), env_ids == NULL (envs 0..m-1, needs m == N), an id outside
 *     [0, N) (skipped: nothing of an env is read, no output row of it is written), m == 0 (does nothing), the 16-byte alignment of obs,
 *     rew, final_state and work, SS_LOOK_WORK words of workspace per row.
 * Ordered on `stream`, never synchronises the host, allocates nothing, can be captured into a graph.  Bad host arguments return
 * SS_ERR_INVALID and launch nothing.  A row's bits depend on its id, its state row, the knobs and its actions alone. */
int ss_lookahead_states(ss_env* env, const int32_t* env_ids, int32_t m, const float* states, int32_t horizon,
                        const float* act, float* obs, float* rew, uint8_t* done, float* final_state, float* work,
                        void* stream);

/* Observation of state rows: obs[k, :] (DEVICE [m, 60] f32) is bit for bit ss_get_obs's row of an env after ss_set_state of states[k, :]
 * (DEVICE [m, SS_STATE_DIM] f32) -- the observation at the root of a branch, which ss_lookahead* never returns, and what relabelling a
 * logged state needs.  Added under version 4.  It only reads `states`; the handle supplies the robot kind; an observation depends on no
 * id and no knob.  m >= 0 (0: nothing happens); states and obs are required when m > 0, 4-byte aligned.  Ordered on `stream`, never
 * synchronises the host, allocates nothing, can be captured into a graph.  Bad host arguments return SS_ERR_INVALID and launch nothing. */
int ss_get_obs_states(ss_env* env, int32_t m, const float* states, float* obs, void* stream);

/* Closed-loop look-ahead (docs/PHYSICS.md 14 "Branches under a policy"); added under version 4 (nothing existing moved).  The actions
 * of a branch come from a small frozen MLP f evaluated inside the launch: with o[k,-1] the observation at the root of branch k (bit for
 * bit ss_get_obs_states of states[k, :], or ss_get_obs of env env_ids[k] when states == NULL) and o[k,s] the observation after step s,
 *     a[k,s] = f(o[k,s-1]) + act_offset[k,s]        (offset 0 without act_offset; f in f32)
 * is the action of step s, which is ss_step's control step under a[k,s] (clipped there; a NaN ends the episode there).
 *
 * The network: `layers` fully connected layers y = activation(W x + b), widths width[0] = 60 (an observation) .. width[layers] = 21 (an
 * action).  ss_policy_words: f32 words of the packed form of such a network, -1 for a description that is not valid.  ss_policy_pack: a
 * device-side repack of the layers' weights (torch's nn.Linear.weight, [out, in] row-major) and biases into `packed`; ordered on
 * `stream`, can be captured into a graph, never synchronises the host; call it again after the weights changed.  weight and bias are
 * HOST arrays of `layers` DEVICE pointers, read during the call only; the arrays they point to are read on the stream.  The packed
 * layout (tiled for the kernel's matrix instructions, zero padded) is OPAQUE: it may change with any release and is valid only for the
 * library that packed it.
 *
 * ss_lookahead_policy: everything not said here is ss_lookahead's / ss_lookahead_states', word for word -- env_ids conventions (NULL:
 * envs 0..m-1, needs m == N; an id outside [0, N) is skipped, nothing of it is written, `act` included), m == 0 does nothing, repeated
 * ids, frozen rows behind a first done, the time limit, the 16-byte alignment of obs, rew, final_state and work (act and act_offset:
 * 4-byte), SS_LOOK_WORK words of workspace per row, no host synchronisation, no allocation, capturable.  The env is only read.
 *   states: NULL (each branch starts where its env stands) or DEVICE [m, SS_STATE_DIM] as in ss_lookahead_states.
 *   d, packed: the description and the blob ss_policy_pack wrote for it (16-byte aligned).
 *   act_offset: NULL or DEVICE [m, horizon, 21] f32 (exploration noise, a perturbation sequence of a sampling planner).
 *   act: NULL or DEVICE [m, horizon, 21] f32: a[k,s], unclipped; 0.0f for every step behind the branch's first done.
 * Given the reported actions the physics is ss_lookahead's: obs, rew, done and final_state are bit for bit what ss_lookahead /
 * ss_lookahead_states write for the same rows under `act`.  A row's bits, actions included, depend on its id, its state, the knobs, the
 * policy and its offsets alone: not on N, m, k, on which outputs were asked for, or on the horizon (prefix property as in ss_lookahead).
 * NOT bitwise: f itself against another evaluation of the same network (torch, a CPU build of this library's code): the kernel sums each
 * dot product as one f32 fma chain in index order starting from the bias, others sum in other orders; tanh and the division of softsign
 * may differ by a few ulp between implementations.  tests/test_gpu_lookahead_policy.py holds the difference to 8 x the error of a plain
 * f32 evaluation against fp64; tests/test_policy_ops.py holds the chain itself (bit for bit for identity / relu networks) and every
 * output to its own rounding bound.  f is defined for finite activations: an infinite hidden activation gives either the unpadded
 * network's actions or NaN in every action of the row (docs/PHYSICS.md 14). */
#define SS_POLICY_MAX_LAYERS 8
#define SS_POLICY_MAX_WIDTH  256
enum { SS_POLICY_IDENTITY = 0, SS_POLICY_RELU = 1, SS_POLICY_SOFTSIGN = 2, SS_POLICY_TANH = 3 };
typedef struct {
  int32_t layers;                                   /* 1 .. SS_POLICY_MAX_LAYERS */
  int32_t width[SS_POLICY_MAX_LAYERS + 1];          /* width[0] == 60, width[layers] == 21, others 1 .. SS_POLICY_MAX_WIDTH */
  int32_t activation[SS_POLICY_MAX_LAYERS];         /* one of SS_POLICY_* per layer */
} ss_policy_desc;
int64_t ss_policy_words(const ss_policy_desc* d);
int ss_policy_pack(ss_env* env, const ss_policy_desc* d, const float* const* weight, const float* const* bias, float* packed,
                   void* stream);
int ss_lookahead_policy(ss_env* env, const int32_t* env_ids, int32_t m, const float* states, int32_t horizon, const ss_policy_desc* d,
                        const float* packed, const float* act_offset, float* act, float* obs, float* rew, uint8_t* done,
                        float* final_state, float* work, void* stream);

/* Measurement aids (tools/hbm_traffic.py, tools/phase_profile.py); not part of the env protocol.
 * ss_debug_calib_copy: dword-per-lane copy out[i] = in[i] + 1 used to calibrate the HBM PMC counters.
 * ss_debug_phase_cycles: 16 per-phase shader-clock totals (zeros unless built with -DSS_PROFILE_PHASES). */
int ss_debug_calib_copy(const float* in, float* out, uint64_t n, void* stream);
int ss_debug_phase_cycles(ss_env* env, unsigned long long* out16, int reset);
/* Self-check aid: the global id of env e becomes env_id_offset + (e & mask) (default mask: all ones), so that envs e and
 * e + 2^k share their Philox streams; injected with the same state they must come out bit-equal from one launch
 * (tests/test_gpu_first_launch.py, tests/host/first_launch_check.c). */
int ss_debug_set_id_mask(ss_env* env, uint32_t mask);

#ifdef __cplusplus
}
#endif
#endif
