"""Pose-sensitivity export: the counterpart of the reference's nerfuncertainty/scripts/estimate_gradient_pose_6dof.py.

The script perturbs one training camera along one of six pose parameters, renders it in 256-ray chunks and calls
torch.autograd.grad(pred_rgb_j.mean(-1), c2w) once per pixel (:153-190).  Here the per-pixel gradients of a frame come from
one kernel launch per group of rays (models.*.get_pose_gradients_for_camera -> render.pose_gradient_camera ->
unerf_pose_grad; for the splat models -> splat.pose_gradient_camera -> unerf_splat_pose_tangents + unerf_splat_pose_grad),
and the files the script leaves behind are written with its names, shapes and dtypes.  tangent_basis / pose_projection give
the six pose parameters and a pose covariance as a [12,P] projection for the per-channel Jacobians (render.pose_jacobian_camera;
for the splat models splat.pose_jacobian_camera, which maps it through viewmat_jacobian first).

What differs from the reference: it differentiates whatever arithmetic its checkpoint runs in (half precision for a tcnn
field); this build differentiates the fp32 field.  Its ground-truth and rendered images are JPEG (mediapy); no JPEG encoder
is assumed here, the rendered image is a PNG."""
from __future__ import annotations

import copy
from pathlib import Path
from typing import Dict

import numpy as np
import torch

POSE_PARAMS = ("tx", "ty", "tz", "angx", "angy", "angz")


def exp_map_se3(tangent: torch.Tensor) -> torch.Tensor:
    """[UPSTREAM-RECALL nerfstudio 1.1.0 cameras.lie_groups.exp_map_SE3, restated from memory] tangent [B,6] =
    (v, w) -> [B,3,4] = (exp([w]x) | V v): the SE(3) exponential of the twist, with upstream's series for |w| < 1e-2
    (cos ~ 8 / (4 + t^2) - 1, sin t / t ~ (cos + 1) / 2 in the rotation; Taylor terms in the translation)."""
    lin = tangent[:, :3].reshape(-1, 3, 1)
    ang = tangent[:, 3:].reshape(-1, 3, 1)
    theta = torch.linalg.norm(ang, dim=1).unsqueeze(1)
    theta2, theta3 = theta ** 2, theta ** 3
    near_zero = theta < 1e-2
    one = torch.ones(1, dtype=tangent.dtype, device=tangent.device)
    theta_nz, theta2_nz, theta3_nz = (torch.where(near_zero, one, t) for t in (theta, theta2, theta3))
    sine = theta.sin()
    cosine = torch.where(near_zero, 8 / (4 + theta2) - 1, theta.cos())
    sine_by_theta = torch.where(near_zero, 0.5 * cosine + 0.5, sine / theta_nz)
    omc_by_theta2 = torch.where(near_zero, 0.5 * sine_by_theta, (1 - cosine) / theta2_nz)
    ret = torch.zeros(tangent.shape[0], 3, 4, dtype=tangent.dtype, device=tangent.device)
    ret[:, :3, :3] = omc_by_theta2 * ang @ ang.transpose(1, 2)
    for a in range(3):
        ret[:, a, a] += cosine.view(-1)
    temp = sine_by_theta.view(-1, 1) * ang.view(-1, 3)
    ret[:, 0, 1] -= temp[:, 2]
    ret[:, 1, 0] += temp[:, 2]
    ret[:, 0, 2] += temp[:, 1]
    ret[:, 2, 0] -= temp[:, 1]
    ret[:, 1, 2] -= temp[:, 0]
    ret[:, 2, 1] += temp[:, 0]
    sine_by_theta = torch.where(near_zero, 1 - theta2 / 6, sine_by_theta)
    omc_by_theta2 = torch.where(near_zero, 0.5 - theta2 / 24, omc_by_theta2)
    tms_by_theta3 = torch.where(near_zero, 1.0 / 6 - theta2 / 120, (theta - sine) / theta3_nz)
    ret[:, :, 3:] = sine_by_theta * lin
    ret[:, :, 3:] += omc_by_theta2 * torch.cross(ang, lin, dim=1)
    ret[:, :, 3:] += tms_by_theta3 * (ang @ (ang.transpose(1, 2) @ lin))
    return ret


def pose_multiply(pose_a: torch.Tensor, pose_b: torch.Tensor) -> torch.Tensor:
    """[UPSTREAM-RECALL nerfstudio 1.1.0 utils.poses.multiply] [...,3,4] x [...,3,4]: (R1 R2 | t1 + R1 t2)"""
    R1, t1 = pose_a[..., :3, :3], pose_a[..., :3, 3:]
    R2, t2 = pose_b[..., :3, :3], pose_b[..., :3, 3:]
    return torch.cat([R1.matmul(R2), t1 + R1.matmul(t2)], dim=-1)


def perturbed_pose(c2w: torch.Tensor, param: str, magnitude: float) -> torch.Tensor:
    """estimate_gradient_pose_6dof.py:22-39, 118-124: c2w [3,4] times the SE(3) exponential of a twist that is
    `magnitude` in one of tx | ty | tz | angx | angy | angz and zero elsewhere (the camera's own frame) -> [3,4] float32"""
    if param not in POSE_PARAMS:
        raise ValueError(f"shift_param={param!r}: expected one of {', '.join(POSE_PARAMS)}")
    p = torch.zeros(1, 6)
    p[0, POSE_PARAMS.index(param)] = float(magnitude)
    c2w = torch.as_tensor(c2w).detach().cpu().to(torch.float32)
    c2w = c2w[0] if c2w.dim() == 3 else c2w
    return pose_multiply(c2w[:3, :4], exp_map_se3(p)[0])


def tangent_basis(c2w: torch.Tensor) -> torch.Tensor:
    """[12,6] float64: column k = d vec(pose_multiply(c2w, exp_map_se3(xi))) / d xi_k at xi = 0, POSE_PARAMS order, vec
    row-major over the 3x4 pose.  Closed form: a translation along camera axis k moves the origin by c2w[:3,k] (column 3);
    a rotation about camera axis k turns the 3x3 block into c2w[:3,:3] [e_k]x.  c2w[:3,:3] need not be orthogonal."""
    c2w = torch.as_tensor(c2w).detach().cpu().to(torch.float64)
    c2w = (c2w[0] if c2w.dim() == 3 else c2w)[:3, :4]
    Rm = c2w[:, :3]
    B = torch.zeros(3, 4, 6, dtype=torch.float64)
    for k in range(3):
        B[:, 3, k] = Rm[:, k]
        ek = torch.zeros(3, 3, dtype=torch.float64)   # [e_k]x
        ek[(k + 2) % 3, (k + 1) % 3] = 1.0
        ek[(k + 1) % 3, (k + 2) % 3] = -1.0
        B[:, :3, 3 + k] = Rm @ ek
    return B.reshape(12, 6)


def viewmat_jacobian(c2w: torch.Tensor) -> torch.Tensor:
    """[12,12] float64: d vec(V[:3,:4]) / d vec(c2w) at c2w (both row-major over 3x4) for the splat models' world-to-camera
    rows V = [R'^T | -R'^T t], R' = R diag(1,-1,-1) -- the transposition the reference uses, not an inverse, so R need not be
    orthogonal.  Closed form: V[a][b] = F_a R[b][a] and V[a][3] = -F_a sum_r R[r][a] t[r]."""
    c2w = torch.as_tensor(c2w).detach().cpu().to(torch.float64)
    c2w = (c2w[0] if c2w.dim() == 3 else c2w)[:3, :4]
    F = (1.0, -1.0, -1.0)
    J = torch.zeros(12, 12, dtype=torch.float64)
    for a in range(3):
        for r in range(3):
            J[4 * a + r, 4 * r + a] = F[a]
            J[4 * a + 3, 4 * r + a] = -F[a] * c2w[r, 3]
            J[4 * a + 3, 4 * r + 3] = -F[a] * c2w[r, a]
    return J


def splat_view_projection(c2w: torch.Tensor, proj=None, max_p: int = 12) -> torch.Tensor:
    """[12,P] float32: what the splat tangents of ONE view are contracted with -- viewmat_jacobian(c2w) @ proj in float64, then
    rounded (proj [12,P] in c2w entries, as pose_projection gives it; None: the 12 x 12 identity, i.e. d / d c2w).  One 2-D
    product per view, so a view's matrix has the same bits alone (splat.pose_jacobian_camera) and in a batch
    (splat.pose_jacobian_cameras)."""
    M = viewmat_jacobian(c2w)
    if proj is not None:
        pj = torch.as_tensor(proj).detach().cpu().to(torch.float64)
        if pj.dim() != 2 or pj.shape[0] != 12 or not 1 <= pj.shape[1] <= max_p:
            raise ValueError(f"proj must be [12,P] with 1 <= P <= {max_p}, got {tuple(pj.shape)}")
        M = M @ pj
    return M.to(torch.float32)


def pose_projection(c2w: torch.Tensor, pose_cov=None) -> torch.Tensor:
    """[12,P] float64 = tangent_basis(c2w) @ L with L L^T = the [6,6] covariance of the pose parameters (POSE_PARAMS order,
    the camera's own frame): what ops.pose_jacobian(proj=) contracts a d/dc2w row with, so that the sum of squares over P is
    the first-order variance row Sigma row^T.  pose_cov: None -> the basis itself (P = 6: the Jacobian in the six
    parameters); a 6-vector of standard deviations -> a diagonal covariance; a [6,6] symmetric positive semi-definite matrix ->
    its Cholesky factor, a zero pivot's column left out (P = its rank, at least one column)."""
    B = tangent_basis(c2w)
    if pose_cov is None:
        return B
    cov = torch.as_tensor(pose_cov).detach().cpu().to(torch.float64)
    if cov.shape == (6,):
        if bool((cov < 0).any()):
            raise ValueError("pose_projection: a standard deviation is negative")
        L = torch.diag(cov)
    elif cov.shape == (6, 6):
        if not torch.allclose(cov, cov.T, rtol=1e-10, atol=0.0):
            raise ValueError("pose_projection: pose_cov is not symmetric")
        L = torch.zeros(6, 6, dtype=torch.float64)
        tol = 1e-14 * float(cov.diagonal().abs().max())
        for j in range(6):   # Cholesky by columns; a pivot at rounding level ends its column (semi-definite input)
            piv = float(cov[j, j] - (L[j, :j] ** 2).sum())
            if piv < -1e-10 * float(cov.diagonal().abs().max()):
                raise ValueError("pose_projection: pose_cov is not positive semi-definite")
            if piv <= tol:
                continue
            L[j, j] = piv ** 0.5
            L[j + 1:, j] = (cov[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    else:
        raise ValueError(f"pose_projection: pose_cov must be None, [6] or [6,6], got {tuple(cov.shape)}")
    keep = (L != 0).any(dim=0)
    if not bool(keep.any()):
        keep[0] = True   # a zero covariance: one zero column, the variance is exactly 0
    return B @ L[:, keep]


def _sym_eig(information, what: str):
    """a symmetric [P,P] host matrix -> (eigenvalues ascending, eigenvectors) in float64; the two triangles are averaged"""
    H = np.asarray(torch.as_tensor(information).detach().cpu().numpy() if torch.is_tensor(information) else information, np.float64)
    if H.ndim != 2 or H.shape[0] != H.shape[1]:
        raise ValueError(f"{what}: information must be [P,P], got {H.shape}")
    if not np.isfinite(H).all():
        raise ValueError(f"{what}: information holds a non-finite entry")
    return np.linalg.eigh(0.5 * (H + H.T))


def pose_step(information, gradient, damping: float = 0.0, rcond: float = 1e-12):
    """delta = -(H + damping diag H)^-1 g, the Gauss-Newton (damping = 0) or Levenberg-Marquardt step of the weighted
    photometric cost on c2w . exp(xi), from the information and gradient of pose_normal_eq_finish (host, float64).  Solved
    through a symmetric eigendecomposition of the damped matrix: directions with eigenvalue <= rcond * the largest are left at 0
    (a pose direction the frame does not determine gets no step).  -> (delta [P] float64 numpy, numerical rank)"""
    H = np.asarray(information, np.float64)
    g = np.asarray(gradient, np.float64).reshape(-1)
    if damping < 0:
        raise ValueError(f"pose_step: damping = {damping}")
    if H.shape != (g.size, g.size):
        raise ValueError(f"pose_step: information {H.shape} for a gradient of {g.size}")
    lam, Q = _sym_eig(H + float(damping) * np.diag(np.diag(H)), "pose_step")
    keep = lam > rcond * max(float(lam.max(initial=0.0)), 0.0)
    inv = np.where(keep, 1.0 / np.where(keep, lam, 1.0), 0.0)
    return -(Q @ (inv * (Q.T @ g))), int(keep.sum())


def pose_covariance(information, prior=None, rcond: float = 1e-12):
    """The Laplace approximation of the pose posterior: the pseudo-inverse of the information (prior: an optional [P,P]
    prior INFORMATION, the inverse of a prior covariance, added first) on pose_step's rank rule.  -> (covariance [P,P] float64
    numpy, numerical rank).  A full-rank [6,6] result is a valid pose_cov of get_pose_uncertainty_for_camera."""
    H = np.asarray(information, np.float64)
    if prior is not None:
        Pm = np.asarray(torch.as_tensor(prior).detach().cpu().numpy() if torch.is_tensor(prior) else prior, np.float64)
        if Pm.shape != H.shape:
            raise ValueError(f"pose_covariance: prior {Pm.shape} for an information of {H.shape}")
        H = H + Pm
    lam, Q = _sym_eig(H, "pose_covariance")
    keep = lam > rcond * max(float(lam.max(initial=0.0)), 0.0)
    inv = np.where(keep, 1.0 / np.where(keep, lam, 1.0), 0.0)
    cov = (Q * inv) @ Q.T
    return 0.5 * (cov + cov.T), int(keep.sum())


def apply_pose_step(c2w: torch.Tensor, delta) -> torch.Tensor:
    """pose_multiply(c2w, exp_map_se3(delta)): the [3,4] float32 pose after the twist delta [6] (POSE_PARAMS order, the camera's
    own frame) -- perturbed_pose for a general twist"""
    c2w = torch.as_tensor(c2w).detach().cpu().to(torch.float32)
    c2w = (c2w[0] if c2w.dim() == 3 else c2w)[:3, :4]
    d = torch.as_tensor(np.asarray(delta, np.float64).reshape(1, 6)).to(torch.float32)
    return pose_multiply(c2w, exp_map_se3(d)[0])


def refine_pose(info_fn, camera, image, iters: int = 10, damping: float = 1e-3, rcond: float = 1e-12, **info_kwargs):
    """Levenberg-Marquardt on the camera pose against `image`.  info_fn(camera, image=image, **info_kwargs) -> a dictionary with
    "information", "gradient" and "chi2" (models.*.get_pose_information_for_camera / get_splat_pose_information_for_camera).
    Each iteration takes pose_step at the current damping and evaluates the stepped pose: the step is accepted when that
    call's chi2 is lower (damping / 10), else rejected (damping x 10, the pose stays).  The camera is copied, never modified.
    -> {"poses": the accepted poses [3,4] (the first is the camera's own), "chi2": the chi2 of every evaluation with its
    "accepted" flags, "c2w": the final pose, "covariance", "rank": posegrad.pose_covariance of the final pose's information,
    "damping": the final damping}"""
    cam = copy.copy(camera)
    c2w = torch.as_tensor(camera.camera_to_worlds).detach().cpu().to(torch.float32)
    c2w = (c2w[0] if c2w.dim() == 3 else c2w)[:3, :4].clone()
    cam.camera_to_worlds = c2w
    cur = info_fn(cam, image=image, **info_kwargs)
    poses, chi2, accepted = [c2w], [float(cur["chi2"])], [True]
    lam = float(damping)
    for _ in range(int(iters)):
        delta, _rank = pose_step(cur["information"], cur["gradient"], lam, rcond)
        if not np.any(delta):
            break
        trial = apply_pose_step(c2w, delta)
        cam_t = copy.copy(cam)
        cam_t.camera_to_worlds = trial
        nxt = info_fn(cam_t, image=image, **info_kwargs)
        ok = float(nxt["chi2"]) < float(cur["chi2"])
        chi2.append(float(nxt["chi2"]))
        accepted.append(ok)
        if ok:
            c2w, cam, cur = trial, cam_t, nxt
            poses.append(trial)
            lam /= 10.0
        else:
            lam *= 10.0
    cov, rank = pose_covariance(cur["information"], rcond=rcond)
    return {"poses": poses, "chi2": chi2, "accepted": accepted, "c2w": c2w, "covariance": cov, "rank": rank, "damping": lam}


def export_pose_gradients(model, camera, image_idx: int, output_dir, shift_param: str = "tz", shift_magnitude: float = 0.0,
                          seed: int = 42, gradient_fn=None) -> Dict[str, Path]:
    """One image of estimate_gradient_pose_6dof.py:109-216 -> the files it writes under output_dir / f"image_{image_idx}":
      c2w_img{idx}.npy          [3,4] float32    the camera's own pose
      c2w_perturbed.npy         [3,4] float32    perturbed_pose(c2w, shift_param, shift_magnitude)
      camera_intrinsics.npy     [3,3] float32    K
      pred_rgb_perturbed.npy    [H,W,3] float32  the perturbed camera's render (the colour the gradient kernel composited)
      c2w_grads_perturbed.npy   [H,W,3,4] float64  d mean_c(rgb[y,x]) / d c2w_perturbed
      image{idx:05d}_perturbed.png               the render as an 8-bit image (the reference writes a JPEG)
    model: anything with get_pose_gradients_for_camera(camera, want_rgb=True) (models.NerfactoModel / ActiveNerfactoModel,
    models.SplatfactoModel / ActiveSplatfactoModel -- for which the reference's script has no counterpart: it asserts a
    NerfactoModel -- and the plugin's models).  camera: one camera (camera_to_worlds, fx, fy, cx, cy, height, width, ...); it is not modified.
    seed: as the script, torch.manual_seed(seed) before the perturbation (which draws nothing).
    gradient_fn: None, or a callable (camera, want_rgb=True) -> (grads, rgb) used instead of the model's method, e.g.
    model.get_mc_pose_gradients_for_camera or functools.partial of it with a mask_seed, or
    functools.partial(model.get_laplace_pose_gradients_for_camera, generator=g) for the Laplace frame of that draw.
    -> {file stem: path}"""
    from .eval import _write_png
    from .models import _scalar
    torch.manual_seed(seed)
    out = Path(output_dir) / f"image_{int(image_idx)}"
    out.mkdir(parents=True, exist_ok=True)
    c2w = torch.as_tensor(camera.camera_to_worlds).detach().cpu().to(torch.float32)
    c2w = (c2w[0] if c2w.dim() == 3 else c2w)[:3, :4]
    c2w_p = perturbed_pose(c2w, shift_param, shift_magnitude)
    cam = copy.copy(camera)
    cam.camera_to_worlds = c2w_p
    grads, rgb = (model.get_pose_gradients_for_camera if gradient_fn is None else gradient_fn)(cam, want_rgb=True)
    rgb = rgb.detach().cpu().to(torch.float32).numpy()
    K = np.array([[_scalar(camera.fx), 0.0, _scalar(camera.cx)], [0.0, _scalar(camera.fy), _scalar(camera.cy)], [0.0, 0.0, 1.0]],
                 np.float32)
    files = {"c2w": out / f"c2w_img{int(image_idx):d}.npy", "c2w_perturbed": out / "c2w_perturbed.npy",
             "camera_intrinsics": out / "camera_intrinsics.npy", "pred_rgb_perturbed": out / "pred_rgb_perturbed.npy",
             "c2w_grads_perturbed": out / "c2w_grads_perturbed.npy", "image": out / f"image{int(image_idx):05d}_perturbed.png"}
    np.save(files["c2w"], c2w.numpy())
    np.save(files["c2w_perturbed"], c2w_p.numpy())
    np.save(files["camera_intrinsics"], K)
    np.save(files["pred_rgb_perturbed"], rgb)
    np.save(files["c2w_grads_perturbed"], grads.detach().cpu().numpy().astype(np.float64))
    _write_png(files["image"], np.clip(np.rint(rgb * 255.0), 0, 255).astype(np.uint8))
    return files
