"""Batched offline VLA-action labelling of an episode (the throughput-bound consumer of the RDT path).

The reference labels one timestep at a time (data/create_controller_dataset_episode.py:186-205): for every t it pushes the two
camera frames into a 2-deep observation window (the third camera is always None, the slot before the first frame is an all-None
dummy, :50-97) and calls `policy.step(proprio=qpos[t], images=[ext_{t-1}, right_{t-1}, None, ext_t, right_t, None], text_embeds)`
(:99-125) — 6 SigLIP forwards and one batch-1 RDT chunk per timestep.  None of that depends on the model's outputs, so here
  * every distinct frame goes through the SigLIP tower ONCE (a frame serves the windows of t and t+1; the None slots are one cached
    background image): 2 image encodes per timestep instead of 6, in large batches;
  * the RDT chunks of `batch` timesteps are generated together (323 vs 32 chunks/s at batch 32 vs 1 on an MI355X).
Frames are either the `camera{1,2}_resized` arrays the reference's labeller writes (already padded and resized for SigLIP) or, with
`pad_and_resize=True`, the raw `camera1/camera1` frames of an episode: the reference's `pad_and_resize_for_siglip` (:198-199) then runs
first, on the card (csrc/vt_area.hip) with the model's device preprocessing, through the numpy statement without it; both give the pixels
of vlatouch.imgprep.pad_and_resize_for_siglip, UNPINNED against cv2 (see that module).  `return_resized=True` also returns the resized
frames, the `camera{1,2}_resized` arrays `convert.write_labelled_episode` stores.  The reference's cv2 JPEG round trip of every frame
(:53-57, "to align with training") is `jpeg_mapping=True`: on the card (csrc/vt_jpegmap.hip, behind that stage and ahead of the
preprocessor's own resize) with the model's device preprocessing, through Pillow without it; both give the pixels of
vlatouch.jpegmap.jpeg_mapping, which is pinned to libjpeg-turbo and UNPINNED against cv2 itself (see that module).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch


@torch.no_grad()
def encode_frames(model, frames: Sequence, batch: int = 48, jpeg_mapping=False, pad_and_resize=False) -> torch.Tensor:
    """frames: sequence of HxWx3 uint8 arrays / PIL images / None -> SigLIP tokens [n, num_patches, hidden] on the model's device.
    jpeg_mapping: False, True (quality 95) or a quality: the reference's JPEG round trip of every frame that exists.
    pad_and_resize: False, True (the tower's size) or a target size: the reference's `pad_and_resize_for_siglip` of every frame that
    exists, ahead of the mapping."""
    from PIL import Image
    from .imgprep import area_size, pad_and_resize_pil
    from .jpegmap import jpeg_mapped_pil, jpeg_quality
    quality = jpeg_quality(jpeg_mapping)
    target = area_size(pad_and_resize, model.image_processor.size["height"]) if pad_and_resize else None
    out = []
    for i in range(0, len(frames), batch):
        if getattr(model, "device_preprocess", False):
            kw = {} if quality is None else {"jpeg": quality}
            if target is not None:
                kw["area"] = target
            px = model.preprocess_images_device(list(frames[i:i + batch]), **kw)   # raw bytes up in one copy, mapped, resized and normalised on the card
        else:
            pil = [None if f is None else (f if isinstance(f, Image.Image) else Image.fromarray(np.asarray(f))) for f in frames[i:i + batch]]
            px = model.preprocess_images(jpeg_mapped_pil(pad_and_resize_pil(pil, target), quality)).to(model.device, dtype=model.dtype)
        out.append(model.vision_model(px))
    return torch.cat(out, dim=0)


@torch.no_grad()
def label_episode(model, frames_cam1: Sequence, frames_cam2: Sequence, qpos, lang_embeddings: torch.Tensor, *, batch: int = 32,
                  noise: Optional[torch.Tensor] = None, encode_batch: int = 48, jpeg_mapping=False, pad_and_resize=False,
                  return_resized: bool = False):
    """VLA action chunks for every timestep of an episode: [N, horizon, 10] float32 (gripper back in 0..255), what the reference's
    per-timestep loop stores as `vla_action`.

    model: scripts.franka_model_eef.RoboticDiffusionTransformerModel;  frames_cam{1,2}: N frames each (ext / right-wrist camera);
    qpos [N, 10] (utils_eef.converted_ee_pose_with_gripper);  lang_embeddings [1, L, lang_dim] cached instruction embedding;
    noise: optional [N, horizon, action_dim] start noise per timestep (the reference draws it inside predict_action);
    jpeg_mapping: as in `encode_frames` (the reference's labeller maps every frame);
    pad_and_resize: as in `encode_frames`: the frames are raw camera frames, padded and resized first as the reference's labeller does;
    return_resized (needs pad_and_resize): return (vla_action, cam1_resized, cam2_resized), the two uint8 [N, target, target, 3] arrays
    the reference's labeller stores as `camera{1,2}_resized`.  The frames are then resized once, here, and encoded from the result."""
    from .imgprep import area_size
    N = len(frames_cam1)
    assert len(frames_cam2) == N and len(qpos) == N
    dev, dt = model.device, model.dtype
    resized = None
    if return_resized:
        target = area_size(pad_and_resize, model.image_processor.size["height"]) if pad_and_resize else None
        if target is None:
            raise ValueError("label_episode: return_resized needs pad_and_resize")
        resized = [_resize_frames(model, list(fr), target, encode_batch) for fr in (frames_cam1, frames_cam2)]
        frames_cam1, frames_cam2, pad_and_resize = resized[0], resized[1], False
    tok1 = encode_frames(model, list(frames_cam1), encode_batch, jpeg_mapping, pad_and_resize)             # [N, P, D]
    tok2 = encode_frames(model, list(frames_cam2), encode_batch, jpeg_mapping, pad_and_resize)
    bg = encode_frames(model, [None], 1)[0]                                  # the None slots: one background image
    qpos = torch.as_tensor(np.asarray(qpos), dtype=torch.float32, device=dev)
    text = lang_embeddings.to(dev, dtype=dt)
    P, D = bg.shape
    out = []
    for t0 in range(0, N, batch):
        ts = list(range(t0, min(N, t0 + batch)))
        B = len(ts)
        img = torch.empty(B, 6, P, D, dtype=tok1.dtype, device=dev)
        for j, t in enumerate(ts):
            img[j, 0] = tok1[t - 1] if t > 0 else bg                          # window[-2]: previous frame (all None before the first)
            img[j, 1] = tok2[t - 1] if t > 0 else bg
            img[j, 2] = bg
            img[j, 3] = tok1[t]
            img[j, 4] = tok2[t]
            img[j, 5] = bg
        states, mask = model._format_joint_to_state(qpos[ts].unsqueeze(1))     # [B, 1, 128], [B, 128]
        traj = model.policy.predict_action(
            lang_tokens=text.expand(B, -1, -1).contiguous(), lang_attn_mask=torch.ones(B, text.shape[1], dtype=torch.bool, device=dev),
            img_tokens=img.reshape(B, 6 * P, D), state_tokens=states.to(dt), action_mask=mask.unsqueeze(1).to(dt),
            ctrl_freqs=torch.full((B,), float(model.control_frequency), device=dev),
            **({"x_init": noise[ts].to(dev)} if noise is not None else {}))
        out.append(model._unformat_action_to_joint(traj).to(torch.float32).cpu())
    action = torch.cat(out, dim=0).numpy()
    return (action, resized[0], resized[1]) if return_resized else action


def _resize_frames(model, frames: list, target: int, batch: int) -> np.ndarray:
    """`pad_and_resize_for_siglip` of every frame of one camera -> uint8 [N, target, target, 3] on the host: on the card with the model's
    device preprocessing, through the numpy statement without it."""
    from PIL import Image
    from .imgprep import pad_and_resize_device, pad_and_resize_for_siglip
    if any(f is None for f in frames):
        raise ValueError("label_episode: return_resized takes episodes without missing frames")
    if getattr(model, "device_preprocess", False):
        return np.concatenate([pad_and_resize_device(frames[i:i + batch], target, device=model.device).cpu().numpy()
                               for i in range(0, len(frames), batch)], axis=0)
    rgb = lambda f: np.asarray(f.convert("RGB") if isinstance(f, Image.Image) else f)
    return np.stack([pad_and_resize_for_siglip(rgb(f), target) for f in frames], axis=0)
