"""Reading the reference's checkpoints from disk: the data format on the input side of the render path.

`ns-train` writes `<run>/nerfstudio_models/step-<9 digits>.ckpt`, a torch pickle `{"step", "pipeline", "optimizers",
"schedulers", ...}` whose `pipeline` entry is the pipeline's state dict (`_model.` prefix, `module.` under DDP).  The
reference finds and loads them in `models/ensemble/ensemble_utils.py:36-110` (`eval_load_ensemble_checkpoints`): the
latest step unless one is named, member i of an ensemble from the `nerfstudio_models` directory next to its
`config.yml`.  Same rules here, for the Model mirrors of `models.py` (whose `load_state_dict` strips the prefixes and
maps the state-dict names) -- no nerfstudio import, no GPU.
"""
from __future__ import annotations

import os
import re
from pathlib import Path
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch

PathLike = Union[str, os.PathLike]
_STEP = re.compile(r"^step-(\d+)\.ckpt$")


# ---- the LPIPS network a nerfstudio checkpoint carries --------------------------------------------------------------
# nerfstudio models keep `self.lpips = LearnedPerceptualImagePatchSimilarity(normalize=True)` as a submodule, so every
# pipeline state dict holds the AlexNet trunk and the five 1x1 heads under `_model.lpips.net.*` [UPSTREAM-RECALL
# torchmetrics.functional.image.lpips: _LPIPS / Alexnet / NetLinLayer / ScalingLayer; the `lpips` package uses the same
# names with `lins.{i}` next to `lin{i}`].
LPIPS_CONVS = (("slice1.0", (64, 3, 11, 11)), ("slice2.3", (192, 64, 5, 5)), ("slice3.6", (384, 192, 3, 3)),
               ("slice4.8", (256, 384, 3, 3)), ("slice5.10", (256, 256, 3, 3)))
LPIPS_SHIFT = (-0.030, -0.088, -0.188)      # ScalingLayer: registered as non-persistent buffers upstream
LPIPS_SCALE = (0.458, 0.448, 0.450)


@dataclass
class LpipsWeights:
    """The tensors of the LPIPS AlexNet, float32 on the CPU, in torch's layouts: convs[l] = (weight [C_out, C_in, k, k],
    bias [C_out]), lins[l] = the l-th head's weights [C_l] (non-negative in a trained network), shift / scale [3].
    `_device` caches what the two routes read: the convolutions repacked to [K, C_out] per device (ops.lpips_batch) and the
    tensors per device and dtype (metrics.lpips).  The tensors are taken as they are when first used: build a new object
    (or clear `_device`) after changing one."""
    convs: List[Tuple[torch.Tensor, torch.Tensor]]
    lins: List[torch.Tensor]
    shift: torch.Tensor
    scale: torch.Tensor
    _device: Dict[str, object] = field(default_factory=dict, repr=False, compare=False)


def lpips_weights_from_state_dict(state_dict) -> Optional[LpipsWeights]:
    """-> the LPIPS weights a checkpoint carries under `[_model.][module.]lpips.net.*`, or None when the set is not
    complete (no warning: a checkpoint without the network is an ordinary one).  A complete set with a tensor of another
    shape raises RuntimeError naming the key."""
    sd = {}
    for k, v in state_dict.items():
        k = k[len("_model."):] if k.startswith("_model.") else k
        k = k[len("module."):] if k.startswith("module.") else k
        if k.startswith("lpips.net."):
            sd[k[len("lpips.net."):]] = v
    if not sd:
        return None
    found: Dict[str, Tuple[str, torch.Tensor, Tuple[int, ...]]] = {}
    for l, (name, shape) in enumerate(LPIPS_CONVS):
        for leaf, want in (("weight", shape), ("bias", shape[:1])):
            key = f"net.{name}.{leaf}"
            if key not in sd:
                return None
            found[f"conv{l}.{leaf}"] = (key, sd[key], want)
        key = next((k for k in (f"lin{l}.model.1.weight", f"lins.{l}.model.1.weight") if k in sd), None)
        if key is None:
            return None
        found[f"lin{l}"] = (key, sd[key], (1, shape[0], 1, 1))
    for name in ("shift", "scale"):
        key = f"scaling_layer.{name}"
        if key in sd:
            found[name] = (key, sd[key], None)
    for key, v, want in found.values():
        if not torch.is_tensor(v) or (want is not None and tuple(v.shape) != want) or (want is None and v.numel() != 3):
            got = tuple(v.shape) if torch.is_tensor(v) else type(v).__name__
            raise RuntimeError(f"lpips.net.{key}: shape {got} in the checkpoint, expected {want or '3 values'}")
    f32 = lambda name: found[name][1].detach().to("cpu", torch.float32).contiguous().clone()
    return LpipsWeights(convs=[(f32(f"conv{l}.weight"), f32(f"conv{l}.bias")) for l in range(5)],
                        lins=[f32(f"lin{l}").reshape(-1) for l in range(5)],
                        shift=f32("shift").reshape(3) if "shift" in found else torch.tensor(LPIPS_SHIFT, dtype=torch.float32),
                        scale=f32("scale").reshape(3) if "scale" in found else torch.tensor(LPIPS_SCALE, dtype=torch.float32))


def checkpoint_steps(load_dir: PathLike) -> List[int]:
    """steps of the `step-*.ckpt` files in `load_dir`, ascending (ensemble_utils.py:64-66 parses every directory
    entry as one; other files are ignored here instead of raising)"""
    load_dir = Path(load_dir)
    if not load_dir.is_dir():
        raise FileNotFoundError(f"No checkpoint directory found at {load_dir}: checkpoints are generated periodically "
                                "during training")
    return sorted(int(m.group(1)) for m in (_STEP.match(x) for x in os.listdir(load_dir)) if m)


def checkpoint_path(load_dir: PathLike, load_step: Optional[int] = None) -> Tuple[Path, int]:
    """-> (path, step): `load_step` or the latest one (ensemble_utils.py:50-70)"""
    if load_step is None:
        steps = checkpoint_steps(load_dir)
        if not steps:
            raise FileNotFoundError(f"no step-*.ckpt under {load_dir}")
        load_step = steps[-1]
    path = Path(load_dir) / f"step-{load_step:09d}.ckpt"
    if not path.exists():
        raise FileNotFoundError(f"Checkpoint {path} does not exist")
    return path, int(load_step)


def read_pipeline_state(path: PathLike, trust_pickle: Optional[bool] = None) -> Tuple[Dict[str, torch.Tensor], int]:
    """-> (pipeline state dict, step) of one checkpoint file, on the CPU (ensemble_utils.py:71-72).
    Read with torch's safe unpickler (tensors and plain containers only).  The reference calls the unrestricted
    `torch.load(load_path, map_location="cpu")`, which runs whatever a pickle asks for; that is available here only as
    an explicit choice -- `trust_pickle=True` or UNERF_TRUST_CHECKPOINT_PICKLE=1 -- and only after the safe unpickler
    has refused the file's CONTENT (pickle.UnpicklingError: older nerfstudio versions stored config objects next to
    the tensors); I/O errors and corrupt files are reported as they are."""
    import pickle
    if trust_pickle is None:
        trust_pickle = os.environ.get("UNERF_TRUST_CHECKPOINT_PICKLE", "0") == "1"
    try:
        state = torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:
        if not trust_pickle:
            raise pickle.UnpicklingError(
                f"{path}: holds objects the safe unpickler refuses ({e}); pass trust_pickle=True (or set "
                "UNERF_TRUST_CHECKPOINT_PICKLE=1) to unpickle a checkpoint you trust") from e
        state = torch.load(path, map_location="cpu", weights_only=False)
    if "pipeline" not in state:
        raise KeyError(f"{path}: no 'pipeline' entry (keys: {sorted(state)})")
    return state["pipeline"], int(state.get("step", -1))


def load_model(model, load_dir: PathLike, load_step: Optional[int] = None, strict: bool = False) -> Tuple[Path, int]:
    """Load one Model mirror from a `nerfstudio_models` directory.  -> (path loaded, step).  Raises (RuntimeError from
    the model's load_state_dict, with the path added) when the checkpoint does not cover the model's parameters: a
    run of another method, implementation or key layout must not render from random weights.  The load report
    (models.IncompatibleKeys: ignored keys, tensor counts) is kept as `model.last_load_report`."""
    path, step = checkpoint_path(load_dir, load_step)
    sd, saved_step = read_pipeline_state(path)
    try:
        report = model.load_state_dict(sd, strict=strict)
    except RuntimeError as e:
        raise RuntimeError(f"{path}: {e}") from e
    try:
        model.last_load_report = report
    except Exception:   # a frozen / slotted model object: the report is informational
        pass
    return path, saved_step if saved_step >= 0 else step


def member_checkpoint_dir(config_path: PathLike) -> Path:
    """`<run>/config.yml` -> `<run>/nerfstudio_models` (ensemble_utils.py:78)"""
    return Path(config_path).parent / "nerfstudio_models"


def load_ensemble(models: Sequence, config_paths: Iterable[PathLike], load_step: Optional[int] = None) -> List[Tuple[Path, int]]:
    """Member i from the checkpoint directory next to config_paths[i] (`eval_load_ensemble_checkpoints`,
    ensemble_utils.py:74-108; the reference takes member 0 from `config.load_dir`, which `eval_setup` points at the
    same place).  Under `torchrun` a rank passes only the members it holds, with their config paths."""
    config_paths = list(config_paths)
    if len(config_paths) != len(models):
        raise ValueError(f"{len(models)} models but {len(config_paths)} config paths")
    return [load_model(m, member_checkpoint_dir(c), load_step) for m, c in zip(models, config_paths)]
