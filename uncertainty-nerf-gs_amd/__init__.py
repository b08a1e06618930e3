"""uncertainty-nerf-gs_amd: MI355X-native uncertainty rendering hot path.

Layout
  csrc/       hand-written HIP kernels + the C ABI (include/unerf.h) -> csrc/libunerf.so
  lib.py      ctypes binding of the C ABI (fails loudly when the library is missing)
  ops.py      torch-tensor wrappers, one per C entry point
  render.py   frame-level pipelines (proposal sampling -> field -> composite -> moments)
  fields.py / models.py / ensemble.py
              host-side mirrors of the reference's Field / Model / EnsemblePipeline surface
  metrics.py  ause / auce / psnr / nll (parity metrics)
  splat.py    frame-level splat pipelines: active_splatfacto_outputs(_batch), pose_gradient_camera (the splat pose gradient),
              pose_jacobian_camera (the splat pose Jacobian of r, g, b, accumulation and depth, and the pose variance),
              pose_jacobian_cameras (the same for up to 16 cameras of one image size in shared launches)
  posegrad.py per-pixel camera-pose gradients of a frame (nerfacto and splat models), exported as the reference's
              pose-sensitivity script writes them; tangent_basis / pose_projection: the six pose parameters and a pose
              covariance for the per-channel pose Jacobian (ops.pose_jacobian, render.pose_jacobian_camera); viewmat_jacobian: c2w -> the splat
              models' world-to-camera rows, differentiated; pose_step / pose_covariance / apply_pose_step / refine_pose: the
              Gauss-Newton side of the pose normal equations (ops.pose_normal_eq_*, render / splat.pose_normal_eq_camera)
"""
__version__ = "0.1.0"
