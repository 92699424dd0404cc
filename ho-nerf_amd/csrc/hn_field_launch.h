// The field launchers and size functions that cross a translation unit, declared ONCE (default arguments appear only here):
// defined in hn_field_obj.hip / hn_field_hand.hip (HN_PREC_FP32), hn_field2_obj.hip / hn_field2_hand.hip (HN_PREC_F16X3, HN_PREC_F16)
// and hn_field_bwd.hip; called from hn_api.hip and hn_field_bwd.hip.  Every f16x3 launcher takes the call's options
// (hn_launch_opts.h) as an argument.
#pragma once
#include <functional>

#include "hn_common.h"

namespace hn {

size_t field_obj_workspace_bytes(int n_pts, int n_cus);
size_t field_hand_workspace_bytes(int n_pts, int n_cus);
int launch_field_obj(const hn_field* f, const float* pts, const float* rays_d, int n_pts, int spr, float* sdf, float* grad, float* rgb,
                     float* feat, void* workspace, size_t workspace_bytes, bool full, hipStream_t stream);
int launch_field_hand(const hn_field* f, const float* pts, int n_pts, const float* bt_inv, const float* T_pose, int n_frames,
                      int pts_per_frame, float* sdf, float* grad, float* rgb, float* feat, void* workspace, size_t workspace_bytes, bool full,
                      hipStream_t stream);

namespace v2 {
size_t field2_obj_workspace_bytes(int n_pts, int n_cus);
size_t field2_obj_adj_workspace_bytes(int n_pts, int n_cus);
size_t field2_obj_tape_bytes(int n_pts);
int field2_obj_signal_arrays();
// tape != NULL (full evaluation only): the evaluation keeps its tape there (field2_*_tape_bytes) for a later adjoint launch, instead
// of using the workspace
int launch_field2_obj(const hn_field* f, const float* pts, const float* rays_d, int n_pts, int spr, float* sdf, float* grad, float* rgb,
                      float* feat, void* workspace, size_t workspace_bytes, bool full, hipStream_t stream, const FieldLaunchOpts& lo,
                      void* tape = nullptr, size_t tape_bytes = 0);
// tape != NULL: the adjoint alone from the tape of a taped evaluation of the same points, whose outputs `grad`, `rgb` are passed back in
int launch_field2_obj_adj(const hn_field* f, const float* pts, const float* rays_d, int n_pts, int spr, const float* g_sdf,
                          const float* g_grad, const float* g_rgb, float* g_pts, float* g_rays_d, void* workspace, size_t workspace_bytes,
                          hipStream_t stream, const FieldLaunchOpts& lo, const void* tape = nullptr, const float* grad = nullptr,
                          const float* rgb = nullptr, float* sig = nullptr, size_t sig_pitch = 0, float* gb_out = nullptr);

size_t field2_hand_workspace_bytes(int n_pts, int n_cus);
size_t field2_hand_adj_workspace_bytes(int n_pts, int n_cus);
size_t field2_hand_tape_bytes(int n_pts);
size_t field2_hand_pose_rows_bytes(int n_pts);
int field2_hand_signal_arrays();
int hand_dropped_samples(unsigned long long* n, bool reset);
int launch_field2_hand(const hn_field* f, const float* pts, int n_pts, const float* bt_inv, const float* T_pose, int n_frames,
                       int pts_per_frame, float* sdf, float* grad, float* rgb, float* feat, void* workspace, size_t workspace_bytes, bool full,
                       hipStream_t stream, const FieldLaunchOpts& lo, void* tape = nullptr, size_t tape_bytes = 0);
int launch_field2_hand_adj(const hn_field* f, const float* pts, int n_pts, const float* bt_inv, const float* T_pose, int n_frames,
                           int pts_per_frame, const float* g_sdf, const float* g_grad, const float* g_rgb, float* g_pts, float* g_bt_inv,
                           float* g_T_pose, void* workspace, size_t workspace_bytes, hipStream_t stream, const FieldLaunchOpts& lo,
                           const void* tape = nullptr, const float* grad = nullptr, const float* rgb = nullptr, float* sig = nullptr,
                           size_t sig_pitch = 0, float* gb_out = nullptr);
}  // namespace v2

namespace bwd {
// mid (with g_params only): called once the forward tape stands (z8 [n,257]: column 0 = sdf * scale, then the feature
// vector; d sdf / d pts [n,3]; the colour network's pre-sigmoid output [n,3]) and before any upstream gradient is read:
// the caller derives g_sdf / g_grad / g_rgb from these values there (hn_render_single_bwd: alpha stage and compositing
// and their adjoints), so a training step's backward pass does not evaluate the field a second time.
typedef std::function<int(const float* z8, const float* grad, const float* rgb_pre)> MidHook;
// ... and for the fused form of the parameter-gradient path: the taped evaluation's outputs themselves (sdf [n], d sdf / d pts [n,3],
// rgb [n,3])
typedef std::function<int(const float* sdf, const float* grad, const float* rgb)> MidHook2;
size_t field_bwd_workspace_bytes(const hn_field* f, int n);
// tape / grad / rgb (HN_PREC_F16X3 only, may be NULL): the tape a taped evaluation of the same points left and that
// evaluation's outputs -- the adjoint then runs alone instead of re-evaluating the field first.  Every field launch inside takes `lo`.
int field_eval_bwd(const hn_field* f, const float* pts, const float* rays_d, int n, int spr, const float* bt_inv, const float* T_pose,
                   int n_frames, int pts_per_frame, const float* g_sdf, const float* g_grad, const float* g_rgb, float* g_pts,
                   float* g_rays_d, float* g_bt_inv, float* g_T_pose, void* workspace, size_t workspace_bytes, hipStream_t s,
                   const FieldLaunchOpts& lo, const void* tape, const float* grad, const float* rgb, float* g_params = nullptr,
                   const MidHook* mid = nullptr, const MidHook2* mid2 = nullptr, const float* sdf_t = nullptr, const float* feat_t = nullptr);
}  // namespace bwd

}  // namespace hn
