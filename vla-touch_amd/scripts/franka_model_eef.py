"""Mirror of /root/reference/VLA/scripts/franka_model_eef.py (RoboticDiffusionTransformerModel, :38-313): the RDT wrapper used on
the robot and by the offline labeller — image padding / preprocessing, SigLIP encoding of the 6 frames, 10-d <-> 128-d state
packing, `predict_action`.  Same constructor, `get_policy`, `reset`, `load_pretrained_weights`,
`_format_joint_to_state`, `_unformat_action_to_joint` and `step(proprio, images, text_embeds)`; the SigLIP tower and the RDT
policy are the HIP-backed mirrors.  Differences, all forced by what is absent here:
  * `configs/state_vec.py` is not in the reference tree: the 10 unified-vector slots come from `state_indices=` (default: upstream
    RDT's mapping eef_pos_{x,y,z} = 30..32, eef_angle_0..5 = 33..38, right_gripper_open = 10 [assumed-upstream]);
  * no torchvision: `transforms.Resize` / `ColorJitter(brightness=1.75)` are done with PIL (same resampling / the same
    ImageEnhance.Brightness torchvision itself uses for PIL images); the SiglipImageProcessor arithmetic (bicubic resize to
    image_size, x/255, (x-0.5)/0.5) is restated in `SiglipPreprocessor` and pinned against HF's PIL processor in tests;
  * the T5 text encoder is optional, as in the reference (which comments it out "due to limited GPU memory"): with `text_model=` /
    `text_tokenizer=` or `pretrained_text_encoder_name_or_path=` it runs on the card (vlatouch.t5) and `encode_instruction` works;
    without one, `encode_instruction` raises NotImplementedError;
  * `step` turns the camera frames into `pixel_values` on the card (`preprocess_images_device`, vlatouch.imgprep): bit-identical to
    `preprocess_images(...).to(device, dtype)`, which stays as the CPU statement and runs when `device_preprocess=False`."""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np
import torch

from models.multimodal_encoder.siglip_encoder import SiglipVisionTower
from models.rdt_runner import RDTRunner
from vlatouch.imgprep import area_size, pad_and_resize_pil
from vlatouch.jpegmap import jpeg_mapped_pil, jpeg_quality

# eef_pos_x, eef_pos_y, eef_pos_z, eef_angle_0..5, right_gripper_open in upstream RDT's configs/state_vec.py [assumed-upstream]
DEFAULT_STATE_INDICES = [30, 31, 32, 33, 34, 35, 36, 37, 38, 10]


class SiglipPreprocessor:
    """SiglipImageProcessor.preprocess for one PIL image: RGB, bicubic resize to (size, size), /255, (x - mean) / std."""

    def __init__(self, size: int = 384, image_mean=(0.5, 0.5, 0.5), image_std=(0.5, 0.5, 0.5)):
        self.size = {"height": size, "width": size}
        self.image_mean, self.image_std = list(image_mean), list(image_std)
        self.rescale_factor = 1 / 255.0

    def preprocess(self, image, return_tensors="pt"):
        from PIL import Image
        image = image.convert("RGB").resize((self.size["width"], self.size["height"]), resample=Image.BICUBIC)
        x = np.asarray(image, dtype=np.float32) * np.float32(self.rescale_factor)
        x = (x - np.asarray(self.image_mean, dtype=np.float32)) / np.asarray(self.image_std, dtype=np.float32)
        return {"pixel_values": torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))[None]}


def create_model(args, **kwargs):
    model = RoboticDiffusionTransformerModel(args, **kwargs)
    pretrained = kwargs.get("pretrained", None)
    if pretrained is not None and os.path.isfile(pretrained):
        model.load_pretrained_weights(pretrained)
    return model


class RoboticDiffusionTransformerModel(object):
    def __init__(self, args, device="cuda", dtype=torch.bfloat16, image_size=None, control_frequency=25, pretrained=None,
                 pretrained_vision_encoder_name_or_path=None, *, vision_model=None, policy=None,
                 state_indices: Optional[Sequence[int]] = None, text_model=None, text_tokenizer=None,
                 pretrained_text_encoder_name_or_path=None, device_preprocess: bool = True):
        self.args = args
        self.device_preprocess = device_preprocess      # frames -> pixel_values on the card (vlatouch.imgprep); False: the PIL path
        self._imgprep = {}
        self.dtype = dtype
        self.image_size = image_size
        self.device = device
        self.control_frequency = control_frequency
        self.state_indices = list(state_indices) if state_indices is not None else list(DEFAULT_STATE_INDICES)
        if vision_model is not None:
            self.vision_model = vision_model
        else:
            self.vision_model = SiglipVisionTower(vision_tower=pretrained_vision_encoder_name_or_path, args=None, device=device,
                                                  precision="bf16" if dtype == torch.bfloat16 else "fp32")
        self.text_tokenizer, self.text_model = text_tokenizer, text_model
        if text_model is None and pretrained_text_encoder_name_or_path is not None:
            self.text_tokenizer, self.text_model = self.get_text_encoder(pretrained_text_encoder_name_or_path)
            if text_tokenizer is not None:
                self.text_tokenizer = text_tokenizer
        self.image_processor = SiglipPreprocessor(self.vision_model.config.image_size)
        self.policy = policy if policy is not None else self.get_policy(pretrained)
        self.reset()

    def get_policy(self, pretrained):
        if pretrained is None or os.path.isfile(pretrained):
            a = self.args
            n_patch = self.vision_model.num_patches
            img_cond_len = a["common"]["img_history_size"] * a["common"]["num_cameras"] * n_patch
            return RDTRunner(
                action_dim=a["common"]["state_dim"], pred_horizon=a["common"]["action_chunk_size"], config=a["model"],
                lang_token_dim=a["model"]["lang_token_dim"], img_token_dim=a["model"]["img_token_dim"],
                state_token_dim=a["model"]["state_token_dim"], max_lang_cond_len=a["dataset"]["tokenizer_max_length"],
                img_cond_len=img_cond_len,
                img_pos_embed_config=[("image", (a["common"]["img_history_size"], a["common"]["num_cameras"], -n_patch))],
                lang_pos_embed_config=[("lang", -a["dataset"]["tokenizer_max_length"])],
                dtype=self.dtype, device=self.device)
        return RDTRunner.from_pretrained(pretrained)

    def reset(self):
        self.policy.eval()
        self.vision_model.eval()

    def load_pretrained_weights(self, pretrained=None):
        if pretrained is None:
            return
        filename = os.path.basename(pretrained)
        if filename.endswith(".pt"):
            self.policy.load_state_dict(torch.load(pretrained, map_location="cpu")["module"])
        elif filename.endswith(".safetensors"):
            from safetensors.torch import load_file
            self.policy.load_state_dict(load_file(pretrained))
        else:
            raise NotImplementedError(f"Unknown checkpoint format: {pretrained}")

    def get_text_encoder(self, pretrained_text_encoder_name_or_path):
        """franka_model_eef.py:115-121: (tokenizer, model) of a T5Embedder; the encoder runs on the card (vlatouch.t5)."""
        from models.multimodal_encoder.t5_encoder import T5Embedder
        embedder = T5Embedder(from_pretrained=pretrained_text_encoder_name_or_path, model_max_length=self.args["dataset"]["tokenizer_max_length"],
                              device=self.device, torch_dtype=self.dtype)
        return embedder.tokenizer, embedder.model

    def encode_instruction(self, instruction, device="cuda"):
        """franka_model_eef.py:145-165: instruction string -> [1, L, d_model] T5 embeddings."""
        if self.text_model is None or self.text_tokenizer is None:
            raise NotImplementedError("no T5 text encoder was given (text_model= / text_tokenizer= or pretrained_text_encoder_name_or_path=): "
                                      "pass cached instruction embeddings to step()")
        tokens = self.text_tokenizer(instruction, return_tensors="pt", padding="longest", truncation=True)["input_ids"].to(device)
        tokens = tokens.view(1, -1)
        with torch.no_grad():
            pred = self.text_model(tokens).last_hidden_state.detach()
        return pred

    def _format_joint_to_state(self, joints):
        """[B, N, 10] EEF proprioception (gripper 0..255) -> unified state [B, N, state_token_dim] and its element mask [B, dim]."""
        joints = joints / torch.tensor([[[1, 1, 1, 1, 1, 1, 1, 1, 1, 255]]], device=joints.device, dtype=joints.dtype)
        B, N, _ = joints.shape
        dim = self.args["model"]["state_token_dim"]
        state = torch.zeros((B, N, dim), device=joints.device, dtype=joints.dtype)
        state[:, :, self.state_indices] = joints
        mask = torch.zeros((B, dim), device=joints.device, dtype=joints.dtype)
        mask[:, self.state_indices] = 1
        return state, mask

    def _unformat_action_to_joint(self, action):
        joints = action[:, :, self.state_indices]
        return joints * torch.tensor([[[1, 1, 1, 1, 1, 1, 1, 1, 1, 255]]], device=joints.device, dtype=joints.dtype)

    def preprocess_images(self, images):
        """franka_model_eef.py:242-281: None -> background image, optional resize, optional brightness lift, pad to square with
        the processor's mean colour, SiglipImageProcessor.preprocess.  Returns pixel_values [n, 3, S, S] fp32."""
        from PIL import Image, ImageEnhance
        mean255 = tuple(int(x * 255) for x in self.image_processor.image_mean)
        S = self.image_processor.size
        background = Image.fromarray(np.ones((S["height"], S["width"], 3), dtype=np.uint8) * np.array(mean255, dtype=np.uint8).reshape(1, 1, 3))
        out = []
        for image in images:
            if image is None:
                image = background
            if self.image_size is not None:
                sz = self.image_size
                if isinstance(sz, int):          # transforms.Resize(int): shorter side -> sz, bilinear
                    w, h = image.size
                    nw, nh = (sz, max(1, int(sz * h / w))) if w <= h else (max(1, int(sz * w / h)), sz)
                    image = image.resize((nw, nh), resample=Image.BILINEAR)
                else:
                    image = image.resize((sz[1], sz[0]), resample=Image.BILINEAR)
            if self.args["dataset"].get("auto_adjust_image_brightness", False):
                px = np.asarray(image.convert("RGB"), dtype=np.float64)
                if px.sum() / (px.shape[0] * px.shape[1] * 255.0 * 3) <= 0.15:
                    image = ImageEnhance.Brightness(image).enhance(1.75)
            if self.args["dataset"].get("image_aspect_ratio", "pad") == "pad":
                w, h = image.size
                if w != h:
                    side = max(w, h)
                    sq = Image.new(image.mode, (side, side), mean255)
                    sq.paste(image, (0, (w - h) // 2) if w > h else ((h - w) // 2, 0))
                    image = sq
            out.append(self.image_processor.preprocess(image, return_tensors="pt")["pixel_values"][0])
        return torch.stack(out, dim=0)

    def preprocess_images_device(self, images, out=None, jitter=None, jpeg=None, corrupt=None, area=None):
        """`preprocess_images(images).to(self.device, self.dtype)`, bit for bit, computed on the card (csrc/vt_imgprep.hip): frames go up
        as raw bytes in one copy; device-resident uint8 [H, W, 3] tensors are used in place.  Per frame: PIL image, HxWx3 uint8 array,
        uint8 tensor (host or device) or None.  `jitter`: per frame None or a vlatouch.imgaug.ColorJitterParams, the training-time
        colour augmentation between the pre-resize / lift and the pad (train/dataset.py:385-391); not part of `preprocess_images`.
        `jpeg`: None or the quality of the reference's cv2 JPEG round trip of every frame that exists (vlatouch.jpegmap), ahead of all
        else; equals `preprocess_images_device([jpeg_mapping(f, jpeg) ...])`.  `corrupt`: per frame None or a vlatouch.imgaug.CorruptParams,
        the training-time corruption directly behind the jitter (train/dataset.py:392-393).  `area`: None or the target size of the
        reference's `pad_and_resize_for_siglip` of every frame that exists (vlatouch.imgprep), ahead of the JPEG mapping; equals
        `preprocess_images_device([pad_and_resize_for_siglip(f, area) ...], jpeg=jpeg)`."""
        from vlatouch.imgprep import DevicePreprocessor
        p, d = self.image_processor, self.args["dataset"]
        size = p.size["height"]
        if p.size["width"] != size:
            raise NotImplementedError("device preprocessing takes a square processor size; use preprocess_images")
        sz = self.image_size if self.image_size is None or isinstance(self.image_size, int) else tuple(int(v) for v in self.image_size)
        key = (size, tuple(p.image_mean), tuple(p.image_std), p.rescale_factor, str(self.device), self.dtype,
               d.get("image_aspect_ratio", "pad") == "pad", bool(d.get("auto_adjust_image_brightness", False)), sz)
        pp = self._imgprep.get(key)
        if pp is None:
            pp = DevicePreprocessor(size, p.image_mean, p.image_std, self.device, self.dtype, pad=key[6], brightness=key[7], image_size=sz,
                                    rescale_factor=p.rescale_factor)
            self._imgprep = {key: pp}
        return pp(list(images), out=out, jitter=jitter, jpeg=jpeg, corrupt=corrupt, area=area)

    @torch.no_grad()
    def step(self, proprio, images, text_embeds, jpeg_mapping=False, pad_and_resize=False):
        """proprio [1, 10]; images: [ext_{t-1}, right_wrist_{t-1}, left_wrist_{t-1}, ext_t, right_wrist_t, left_wrist_t] (PIL or
        None); text_embeds [1, L, lang_token_dim].  Returns the action chunk [1, horizon, 10] fp32 (gripper back in 0..255).
        `jpeg_mapping`: pass every frame through the JPEG round trip the reference's robot loop applies before it calls step
        (frank_inference_eef.py:84-87; vlatouch.jpegmap): False, True (quality 95, cv2's default) or a quality.
        `pad_and_resize`: give step the raw camera frames and let it apply `pad_and_resize_for_siglip` first, as the robot loop does ahead
        of the mapping (frank_inference_eef.py:324-325; vlatouch.imgprep): False, True (the tower's size) or a target size."""
        device, dtype = self.device, self.dtype
        quality = jpeg_quality(jpeg_mapping)
        target = area_size(pad_and_resize, self.image_processor.size["height"])
        if self.device_preprocess:
            image_tensor = self.preprocess_images_device(images, jpeg=quality, area=target)
        else:
            image_tensor = self.preprocess_images(jpeg_mapped_pil(pad_and_resize_pil(images, target), quality)).to(device, dtype=dtype)
        image_embeds = self.vision_model(image_tensor).detach()
        image_embeds = image_embeds.reshape(-1, self.vision_model.hidden_size).unsqueeze(0)
        joints = proprio.to(device).unsqueeze(0)
        states, mask = self._format_joint_to_state(joints)
        states, mask = states.to(device, dtype=dtype), mask.to(device, dtype=dtype)
        states = states[:, -1:, :]
        ctrl_freqs = torch.tensor([self.control_frequency]).to(device)
        text_embeds = text_embeds.to(device, dtype=dtype)
        trajectory = self.policy.predict_action(
            lang_tokens=text_embeds, lang_attn_mask=torch.ones(text_embeds.shape[:2], dtype=torch.bool, device=text_embeds.device),
            img_tokens=image_embeds, state_tokens=states, action_mask=mask.unsqueeze(1), ctrl_freqs=ctrl_freqs)
        return self._unformat_action_to_joint(trajectory).to(torch.float32)
