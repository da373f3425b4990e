"""Python surface of the backend: a mirror of the reference's `AnyRefForCausalLM`
(`model/anyref.py:182-237,647-822`) over the C-ABI library.

What is preserved: the `generate(...)` and `forward(**kwargs)` signatures and
argument meaning, the `[SEG]`-token -> SAM prompt hand-off, the state_dict weight names, the
`.config.{eos,bos,pad}_token_id` attributes and the no-op plumbing calls the eval scripts make
(`get_model()`, `initialize_vision_modules`, `initialize_anyref_modules`,
`resize_token_embeddings`, `.eval()`, `.cuda()`, `.to()`, `.half()`), so
`eval_referseg.py:137` / `eval_avs_object.py:137` can drive this class unchanged.

Deviations, both deliberate:
  * `generate` always returns the 3-tuple `(output_ids, pred_masks, (None, None, None))`; the
    reference returns a 2-tuple on its success path (`anyref.py:822`) but both north-star callers
    unpack three values (`eval_referseg.py:136`, `eval_avs_object.py:137`).
  * batched calls decode every row exactly as a batch of one (per-row lengths, no left-pad
    position shift); left-padded `input_ids` + `attention_masks` are accepted and un-padded here.

PyTorch is only the owner of device memory and streams; all arithmetic runs in libanyref_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

from . import _lib
from .config import (AnyRefConfig, IMAGE_TOKEN_INDEX, AUDIO_REF_INDEX, IMG_REF_INDEX, AUDIO_REF_NUM)

_DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _c_config(cfg: AnyRefConfig, mode: int, max_batch: int, max_seg: int) -> _lib.AnyrefConfig:
    c = _lib.AnyrefConfig()
    c.abi_version = _lib.ABI_VERSION
    c.mode = mode
    cl, l, s = cfg.clip, cfg.llm, cfg.sam
    c.clip_image, c.clip_patch, c.clip_dim, c.clip_heads = cl.image_size, cl.patch, cl.dim, cl.heads
    c.clip_layers_run, c.clip_mlp, c.clip_eps = cl.layers_run, cl.mlp, cl.eps
    c.llm_vocab, c.llm_dim, c.llm_heads, c.llm_layers = l.vocab, l.dim, l.heads, l.layers
    c.llm_mlp, c.llm_max_seq, c.llm_rms_eps, c.llm_rope_theta = l.mlp, l.max_seq, l.rms_eps, l.rope_theta
    c.sam_img, c.sam_patch, c.sam_dim, c.sam_depth = s.img_size, s.patch, s.dim, s.depth
    c.sam_heads, c.sam_mlp_ratio, c.sam_window = s.heads, s.mlp_ratio, s.window
    assert len(s.global_idx) <= 8
    c.sam_n_global = len(s.global_idx)
    for i, g in enumerate(s.global_idx):
        c.sam_global_idx[i] = g
    c.sam_out_chans, c.dec_heads, c.dec_mlp, c.dec_depth = s.out_chans, s.dec_heads, s.dec_mlp, s.dec_depth
    c.num_mask_tokens = s.num_mask_tokens
    c.out_dim, c.audio_dim = cfg.out_dim, cfg.audio_dim
    c.seg_lo, c.seg_hi = cfg.seg_range()
    c.rephrase_weight = float(cfg.rephrase_weight)
    c.max_batch, c.max_seg = max_batch, max_seg
    at = cfg.audio_trunk
    if at is not None:
        c.aud_dim, c.aud_blocks, c.aud_heads, c.aud_mel = at.dim, at.blocks, at.heads, at.mel_bins
        c.aud_len, c.aud_kernel, c.aud_stride, c.aud_clips = at.target_len, at.kernel, at.stride, at.clips
    return c


_NEEDS_HANDLE = frozenset({
    "generate", "model_forward_new", "forward", "__call__", "encode_images", "sam_encode", "mask_decode", "llm_forward",
    "seg_tail", "postprocess", "audio_encode", "device_bytes", "inexact_weights", "set_overlap", "set_early_tail", "set_graphs", "profile_enable", "profile_read",
    "stamps_enable", "stamps_read", "set_side_share", "llm_extend", "set_draft", "draft_stats", "image_session", "session_pool",
    "set_rephrase_paths", "early_masks_done", "load_adapter", "set_adapter", "set_token_scores", "last_token_scores",
    "set_mask_reports", "last_mask_reports", "set_spatial_prompts", "refine", "refine_embedding"})

# the tensors an adapter's `modules_to_save` may carry (train.py:375-387) and anyref_update_weight replaces on a live handle
_SAVED_EXACT = ("model.embed_tokens.weight", "lm_head.weight", "model.text_hidden_fcs.0.0.weight",
                "model.text_hidden_fcs.0.0.bias", "model.text_hidden_fcs.0.2.weight", "model.text_hidden_fcs.0.2.bias",
                "model.audio_projector.weight", "model.audio_projector.bias")
_SAVED_PREFIXES = tuple("model.visual_model.mask_decoder." + p for p in
                        ("mask_tokens.weight", "output_upscaling.0.", "output_upscaling.1.", "output_upscaling.3.",
                         "output_hypernetworks_mlps."))


def is_replaceable(name: str) -> bool:
    """whether `set_adapter` can replace this tensor on a built model (anyref_update_weight's list)"""
    return name in _SAVED_EXACT or name.startswith(_SAVED_PREFIXES)


class AnyRefForCausalLM:
    """MI355X-native stand-in for `model.anyref.AnyRefForCausalLM` (inference surface)."""

    def __init__(self, cfg: AnyRefConfig, mode: str = "perf", device: int = 0, max_batch: int = 1,
                 max_seg: int = 4, audio_encoder=None, defer: bool = False, adapters=None, **kwargs):
        # constructor kwargs of the reference (anyref.py:188-209) that shape the path
        if "seg_token_idx" in kwargs:
            cfg.seg_token_idx = kwargs.pop("seg_token_idx")
        if "rephrase_weight" in kwargs:
            cfg.rephrase_weight = kwargs.pop("rephrase_weight")
        if "out_dim" in kwargs:
            cfg.out_dim = kwargs.pop("out_dim")
        self.ce_loss_weight = kwargs.pop("ce_loss_weight", 1.0)
        self.dice_loss_weight = kwargs.pop("dice_loss_weight", 0.5)
        self.bce_loss_weight = kwargs.pop("bce_loss_weight", 2.0)
        self.vision_pretrained = kwargs.pop("vision_pretrained", None)
        self.add_audio_encoder = bool(kwargs.pop("add_audio_encoder", False))
        self.imagebind_ckpt = kwargs.pop("imagebind_ckpt", "model/ImageBind/imagebind_huge.pth")
        self.cfg = cfg
        self.mode = {"parity": _lib.MODE_PARITY, "perf": _lib.MODE_PERF, "perf_fp8w": _lib.MODE_PERF_FP8W,
                     "parity16": _lib.MODE_PARITY16, "perf_f16": _lib.MODE_PERF_F16,
                     "parity16_f16": _lib.MODE_PARITY16_F16, "perf_int4w": _lib.MODE_PERF_INT4W}[mode]
        self.mode_name = mode
        self.device_index = device
        self.device = torch.device("cuda", device)
        self.max_batch, self.max_seg = max_batch, max_seg
        self.audio_encoder = audio_encoder      # PyTorch-ROCm ImageBind audio trunk (anyref_amd.audio)
        self.config = SimpleNamespace(eos_token_id=cfg.eos_token_id, bos_token_id=cfg.bos_token_id,
                                      pad_token_id=cfg.pad_token_id, hidden_size=cfg.llm.dim,
                                      vocab_size=cfg.llm.vocab, use_cache=True, out_dim=cfg.out_dim,
                                      mm_vision_tower=kwargs.pop("vision_tower", "openai/clip-vit-large-patch14"))
        self.h = None
        self._finalized = False
        # `generate` returns the 3-tuple the two north-star callers unpack (eval_referseg.py:136, eval_avs_object.py:137).
        # The reference's success path itself returns 2 values (anyref.py:822), which is what eval_refer_inv.py:135 and
        # eval_coco20i.py:142 unpack: set `model.success_arity = 2` for those scripts.
        self.success_arity = 3
        # adapter hot-swap: `adapters="qv"` (or projection names) makes the handle keep the unmerged base of
        # those LLaMA linears so that `load_adapter` / `set_adapter` can switch LoRA checkpoints on the built model; None
        # (default): nothing is kept and an adapter can only be merged on the host before the build, as ever
        from .lora import parse_targets
        self.adapter_targets = parse_targets(adapters)
        self._adapters: Dict[str, dict] = {}         # load_adapter
        self.active_adapter: Optional[str] = None
        self._base_saved: Dict[str, torch.Tensor] = {}   # host copies of the replaceable tensors as built
        self._saved_active: set = set()              # replaceable tensors that do not hold their built value now
        self._built_shapes: Dict[str, tuple] = {}
        self._draft_policy: Optional[str] = None     # set_draft_policy
        self._last_answers: Optional[List[List[int]]] = None
        self._session_pool = None                    # the SessionPool this model handed out last (told when its slots are ended)
        self._scores_on = False                      # set_token_scores
        self._scores_call = None                     # (rows, max_new_tokens) of the last generating call, read on demand
        self._scores_many = None                     # generate_many: the entries of its calls, in the caller's item order
        self._reports_on = False                     # set_mask_reports
        self._reports_packed = False                 # ... with a packed-mask buffer armed for every mask-producing call
        self._reports_call = None                    # (heights, widths, packed buffer) of the last such call, read on demand
        self._reports_many = None                    # generate_many: the entries of its calls, in the caller's item order
        self._sp_max = 0                             # set_spatial_prompts
        self._refine_ctx = None                      # low-res logits and sizes of the last generating call (refine)
        # `from_pretrained` flow: weights are gathered on the host first (base checkpoint, CLIP tower, SAM file,
        # token-row resize, LoRA merge all happen BEFORE `.cuda()` in the callers) and go to HBM in one build
        self._host_sd: Optional[Dict[str, torch.Tensor]] = {} if defer else None
        if not defer:
            self._create()

    def _create(self):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("AnyRefForCausalLM needs an MI355X: the HIP backend has no CPU fallback")
        h = C.c_void_p()
        cc = _c_config(self.cfg, self.mode, self.max_batch, self.max_seg)
        rc = self.lib.anyref_create(C.byref(cc), self.device_index, C.byref(h))
        if rc != 0:
            raise RuntimeError("anyref_create: " + self.lib.anyref_last_error(None).decode())
        self.h = h
        if self.adapter_targets:
            self._check(self.lib.anyref_adapter_reserve(self.h, self.adapter_targets), "adapter_reserve")

    @property
    def n_img(self) -> int:
        return self.cfg.clip.n_patches

    def _ensure_built(self):
        """Deferred construction: create the handle for the FINAL config and move the gathered weights to HBM."""
        if self.h is not None:
            return
        from .checkpoint import missing_for
        sd = self._host_sd or {}
        audio = any(k.startswith("model.audio_projector.") for k in sd)
        miss = missing_for(self.cfg, sd.keys(), audio)
        if miss:
            raise RuntimeError(f"{len(miss)} weights of the inference path were never loaded, e.g. {miss[:4]} "
                               "(from_pretrained -> initialize_vision_modules -> initialize_anyref_modules -> adapter)")
        self.config.vocab_size = self.cfg.llm.vocab
        self._create()
        self.load_state_dict(sd)
        self._host_sd = None

    # ---- lifetime ------------------------------------------------------------------------
    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                self.lib.anyref_destroy(h)
            except Exception:
                pass
            self.h = None

    def __getattribute__(self, name):
        # any method that talks to the C-ABI handle first makes sure a deferred build has happened
        if name in _NEEDS_HANDLE:
            object.__getattribute__(self, "_ensure_built")()
        return object.__getattribute__(self, name)

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what}: {self.lib.anyref_last_error(self.h).decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- weights (reference state_dict names) --------------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False):
        if self.h is None:                       # deferred build: keep gathering on the host
            self._host_sd.update(sd)
            return [], []
        for name, t in sd.items():
            if t.dtype not in _DT:
                t = t.float()
            t = t.contiguous()
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            self._check(self.lib.anyref_set_weight(self.h, name.encode(), _ptr(t), int(t.is_cuda), _DT[t.dtype],
                                                   shape, t.dim()), f"set_weight({name})")
        self._check(self.lib.anyref_finalize(self.h), "finalize")
        self._finalized = True
        if self.adapter_targets:                 # what an adapter without these tensors, or set_adapter(None), restores
            self._built_shapes = {k: tuple(v.shape) for k, v in sd.items()}
            self._base_saved = {k: v.detach().to("cpu", copy=True) for k, v in sd.items() if is_replaceable(k)}
        return [], []

    @classmethod
    def from_state_dict(cls, cfg: AnyRefConfig, sd, **kw) -> "AnyRefForCausalLM":
        if cfg.audio_trunk is None and any(k.startswith("model.audio_encoder.modality_trunks.audio.") for k in sd):
            from .config import AudioTrunkConfig          # the checkpoint carries the ImageBind trunk: run it in HIP
            cfg.audio_trunk = AudioTrunkConfig(
                dim=sd["model.audio_encoder.modality_heads.audio.0.weight"].shape[0],
                blocks=1 + max(int(k.split("blocks.")[1].split(".")[0]) for k in sd
                               if k.startswith("model.audio_encoder.modality_trunks.audio.blocks.")))
        m = cls(cfg, **kw)
        m.load_state_dict(sd)
        return m

    # ---- construction path of the reference's callers (eval_referseg.py:62-88) --------------
    @classmethod
    def from_pretrained(cls, model_version: str, torch_dtype=None, mode: Optional[str] = None, device: int = 0,
                        max_batch: int = 1, max_seg: int = 4, max_seq: int = 1024, adapters=None, **model_args):
        """`AnyRefForCausalLM.from_pretrained(model_version, torch_dtype=..., **model_args)` (eval_referseg.py:70-72)
        on an HF `save_pretrained` directory (sharded safetensors / bin): config.json -> LLM shape, every tensor ->
        host state dict under the reference's names.  `model_args` are the reference constructor's kwargs
        (anyref.py:188-209: seg_token_idx, out_dim, vision_pretrained, add_audio_encoder, rephrase_weight, ...).
        The handle is built at `.cuda()` / first use, after the caller's `initialize_*`, `resize_token_embeddings`
        and adapter merge.  `torch_dtype` is accepted for signature parity; the arithmetic type is `mode`
        ("perf" = bf16 storage, fp32 accumulate; "parity" = fp32), default perf.  The reference evaluates in fp16
        (`torch_dtype=torch.float16`), so its checkpoints are fp16: `mode="perf_f16"` (f16 storage, fp32 accumulate, same
        bytes and rate as perf) holds such weights bit for bit, where perf rounds them to bf16 (`inexact_weights` counts
        the elements that changed).  An fp16 checkpoint that has to meet the tolerance bar (identical greedy ids, mask logits
        within 1e-3 of the fp32 forward on the checkpoint's own values) takes `mode="parity16_f16"`: the same exact f16
        storage, every GEMM operand f32 carried as a pair of f16 terms; `parity16` would round such weights to bf16.
        `adapters="qv"` (or a list of projection names) makes the built handle keep the unmerged base of those LLaMA linears, so
        that LoRA checkpoints can be switched on it afterwards (`load_adapter` / `set_adapter`); default None."""
        import json
        import os
        from .checkpoint import read_hf_dir, llm_config_from_hf
        hf = json.load(open(os.path.join(model_version, "config.json")))
        cfg = AnyRefConfig(llm=llm_config_from_hf(hf, max_seq))
        for k in ("eos_token_id", "bos_token_id", "pad_token_id"):
            if hf.get(k) is not None:
                setattr(cfg, k, int(hf[k]))
        model_args.pop("train_mask_decoder", None)
        if "mm_vision_tower" in hf:
            model_args.setdefault("vision_tower", hf["mm_vision_tower"])
        m = cls(cfg, mode=mode or "perf", device=device, max_batch=max_batch, max_seg=max_seg, defer=True, adapters=adapters,
                **model_args)
        m._host_sd.update(read_hf_dir(model_version))
        # a merged checkpoint (merge_lora.py:62 `save_pretrained`) already carries the towers: size them from it
        if "train_mask_decoder" in hf and m.vision_pretrained:
            m._adopt_sam_shape()
        return m

    def _adopt_sam_shape(self):
        from .checkpoint import sam_config_for
        s = self.cfg.sam
        self.cfg.sam = sam_config_for(self.vision_pretrained, img_size=s.img_size, patch=s.patch, window=s.window,
                                      out_chans=s.out_chans)

    def get_model(self):
        return self

    def get_vision_tower(self):
        return self

    def initialize_vision_modules(self, model_args=None, *_a, **_k):
        """LLaVA's `initialize_vision_modules` (eval_referseg.py:77): load the CLIP tower named by
        `config.mm_vision_tower` (a local HF directory) unless the checkpoint already carries it."""
        if self._host_sd is None:
            return None
        from .synth import CLIP_PREFIX
        if any(k.startswith(CLIP_PREFIX) for k in self._host_sd):
            return None
        from .checkpoint import load_clip_tower
        path = getattr(model_args, "mm_vision_tower", None) or self.config.mm_vision_tower
        self.cfg.clip, sd = load_clip_tower(path)
        self._host_sd.update(sd)
        return None

    def initialize_anyref_modules(self, config=None, *_a, **_k):
        """`initialize_anyref_modules` (anyref.py:96-161): SAM from `vision_pretrained` (variant by substring),
        `text_hidden_fcs` and, with `add_audio_encoder`, `audio_projector` freshly initialised as `nn.Linear` does
        (their trained values come with the adapter's `modules_to_save`), ImageBind trunk attached if its file exists."""
        if self._host_sd is None:
            return None
        import os
        from .checkpoint import load_sam
        from .synth import SAM_PREFIX
        sd = self._host_sd
        if self.vision_pretrained is None:
            raise ValueError("initialize_anyref_modules needs the `vision_pretrained` constructor kwarg (anyref.py:98-105)")
        self._adopt_sam_shape()
        if not any(k.startswith(SAM_PREFIX) for k in sd):
            sd.update(load_sam(self.vision_pretrained))
        H, out = self.cfg.llm.dim, self.cfg.out_dim

        def fresh(name, n_out, n_in):
            if name + ".weight" not in sd:
                lin = torch.nn.Linear(n_in, n_out)
                sd[name + ".weight"], sd[name + ".bias"] = lin.weight.detach(), lin.bias.detach()

        fresh("model.text_hidden_fcs.0.0", H, H)
        fresh("model.text_hidden_fcs.0.2", out, H)
        if self.add_audio_encoder:
            fresh("model.audio_projector", H, self.cfg.audio_dim)
            if self.audio_encoder is None:
                from .audio import ImageBindAudio
                self.audio_encoder = ImageBindAudio()
                if os.path.exists(self.imagebind_ckpt):
                    from .checkpoint import read_tensors
                    self.audio_encoder.load_reference_state_dict(read_tensors(self.imagebind_ckpt))
                else:
                    print("ImageBind audio encoder ckpt not found!")
        return None

    def resize_token_embeddings(self, n: int):
        if self._host_sd is None:
            if n != self.cfg.llm.vocab:
                raise ValueError(f"tokenizer has {n} tokens but the backend was built for vocab {self.cfg.llm.vocab}")
            return
        from .checkpoint import resize_token_rows
        resize_token_rows(self._host_sd, n)
        self.cfg.llm.vocab = n
        self.config.vocab_size = n

    def merge_adapter(self, adapter_dir: str):
        """`PeftModel.from_pretrained(model, dir).merge_and_unload()` (anyref_amd.peft_compat)."""
        if self._host_sd is None:
            raise RuntimeError("the LoRA merge happens on the host state dict: call it before .cuda() / first use")
        from .checkpoint import merge_lora
        self.adapter_stats = _HostMergeStats(merge_lora(self._host_sd, adapter_dir), self)
        return self

    # ---- adapter hot-swap on the built model (anyref_adapter_apply / anyref_update_weight) ----
    def load_adapter(self, adapter_dir: str, name: Optional[str] = None) -> str:
        """Parse a peft adapter directory (`checkpoint.read_adapter`), check it against the built shapes and keep it ready:
        lora_A / lora_B as f32 on the device (16 MB per adapter at 7B, rank 8), the `modules_to_save` tensors in pinned host
        memory.  Returns the name `set_adapter` takes (default: the directory's base name).  Needs `adapters=` at
        construction; weights change only at `set_adapter`."""
        if not self.adapter_targets:
            raise RuntimeError("load_adapter: this model keeps no unmerged base to switch adapters on: construct it with "
                               'adapters="qv" (or the projection names), or merge on the host before .cuda()')
        from .checkpoint import read_adapter
        pairs, saved, scaling, fifo = read_adapter(adapter_dir, base_names=self._built_shapes)
        name = name or os.path.basename(os.path.normpath(adapter_dir))
        return self.add_adapter(name, pairs, saved, scaling, fifo)

    def add_adapter(self, name: str, pairs, saved, scaling: float, fan_in_fan_out: bool = False) -> str:
        """`load_adapter` for an adapter already in memory, in `checkpoint.read_adapter`'s terms: `pairs` maps module names
        (`model.layers.0.self_attn.q_proj`) to `(lora_A, lora_B)`, `saved` reference names to `modules_to_save` tensors."""
        if not self.adapter_targets:
            raise RuntimeError('add_adapter: construct the model with adapters="qv" (or the projection names)')
        self._ensure_built()
        from .checkpoint import check_adapter_shapes
        from .lora import device_pair, target_bit, MAX_RANK
        check_adapter_shapes(pairs, saved, self._built_shapes, fan_in_fan_out)
        for mod, (a, _b) in pairs.items():
            if not target_bit(mod + ".weight") & self.adapter_targets:
                raise ValueError(f"adapter targets {mod}.weight, which this model did not reserve (adapters= names "
                                 f"{[k for k, v in _lora_bits().items() if v & self.adapter_targets]})")
            if not 1 <= a.shape[0] <= MAX_RANK:
                raise ValueError(f"{mod}: LoRA rank {a.shape[0]} is outside 1 .. {MAX_RANK}")
        for k in saved:
            if not is_replaceable(k):
                raise ValueError(f"adapter saves {k}, which cannot be replaced on a built model (merge it on the host instead)")
        dev = {}
        for mod, (a, b) in pairs.items():
            da, db = device_pair(a, b, fan_in_fan_out)
            dev[mod + ".weight"] = (da.to(self.device), db.to(self.device))
        pinned = {}
        for k, v in saved.items():
            v = v.detach()
            if v.dtype not in _DT:
                v = v.float()
            v = v.contiguous()
            pinned[k] = v if v.is_cuda else v.pin_memory()
        self._adapters[name] = dict(pairs=dev, saved=pinned, scaling=float(scaling))
        return name

    def _update_weight(self, k: str, t: torch.Tensor):
        if t.dtype not in _DT:
            t = t.float()
        t = t.contiguous()
        shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
        self._check(self.lib.anyref_update_weight(self.h, self._stream(), k.encode(), _ptr(t), int(t.is_cuda), _DT[t.dtype],
                                                  shape, t.dim()), f"update_weight({k})")
        self._slots_ended()

    def _slots_ended(self):
        """the library ended every slot of the session pool (a weight changed): the Python pool forgets its sessions too"""
        if self._session_pool is not None:
            self._session_pool._forget_all()

    def set_adapter(self, name: Optional[str]):
        """Switch the built model to a loaded adapter, or back to the base model with None: every reserved LoRA target becomes
        base + scaling * B A by the rule of `anyref_amd/lora.py` (or its base), the adapter's `modules_to_save` tensors replace
        the built ones and those it does not carry return to their built values.  In place: no rebuild, captured decode
        graphs stay valid.  Ends an open image session, drops a pending draft and forgets the "last" draft memory."""
        if not self.adapter_targets:
            raise RuntimeError('set_adapter: construct the model with adapters="qv" (or the projection names)')
        if name is not None and name not in self._adapters:
            raise KeyError(f"no adapter {name!r} loaded (load_adapter first; loaded: {sorted(self._adapters)})")
        ad = self._adapters[name] if name is not None else dict(pairs={}, saved={}, scaling=1.0)
        keep = []                                    # the name bytes must outlive the call
        arr = (_lib.LoraPair * max(len(ad["pairs"]), 1))()
        for i, (wname, (a, b)) in enumerate(ad["pairs"].items()):
            keep.append(wname.encode())
            arr[i].weight_name, arr[i].A, arr[i].B = keep[-1], a.data_ptr(), b.data_ptr()
            arr[i].r, arr[i].is_device, arr[i].transposed = int(a.shape[0]), 1, 0
        self._last_answers = None
        # (an ImageSession this model handed out is ended by the library: its next use raises "session lost: ended by
        #  anyref_adapter_apply")
        self._check(self.lib.anyref_adapter_apply(self.h, self._stream(), arr, len(ad["pairs"]), float(ad["scaling"])),
                    "adapter_apply")
        self._slots_ended()
        self.active_adapter = name
        for k, v in ad["saved"].items():
            self._update_weight(k, v)
        for k in sorted(self._saved_active - set(ad["saved"])):
            self._update_weight(k, self._base_saved[k])
        self._saved_active = set(ad["saved"])
        return self

    def adapter_stats(self) -> dict:
        """dict(targets_reserved, pairs_active, inexact, last_apply_ms, active_adapter) of `anyref_adapter_stats`:
        `last_apply_ms` is the device time of the last switch's merge launches."""
        self._ensure_built()
        tr, pa, ix, ms = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_double(0.0)
        self._check(self.lib.anyref_adapter_stats(self.h, C.byref(tr), C.byref(pa), C.byref(ix), C.byref(ms)), "adapter_stats")
        return dict(targets_reserved=int(tr.value), pairs_active=int(pa.value), inexact=int(ix.value),
                    last_apply_ms=float(ms.value), active_adapter=self.active_adapter)

    def host_state_dict(self):
        """The gathered weights before the build (deferred construction only)."""
        return self._host_sd

    def eval(self):
        return self

    def cuda(self, *_a):
        self._ensure_built()
        return self

    def half(self):
        return self

    def to(self, *_a, **_k):
        return self

    @property
    def device_bytes(self) -> int:
        return int(self.lib.anyref_device_bytes(self.h))

    @property
    def inexact_weights(self) -> int:
        """Weight elements the handle holds in a value other than the one it was given (anyref_inexact_weights): 0 in
        "parity", 0 in "perf_f16" / "parity16_f16" for an fp16 checkpoint, most elements of that checkpoint in "perf" / "parity16"
        (bf16 storage)."""
        n = C.c_int64(0)
        self._check(self.lib.anyref_inexact_weights(self.h, C.byref(n)), "inexact_weights")
        return int(n.value)

    def set_seg_token_idx(self, seg_token_idx):
        """`seg_token_idx` kwarg of the reference constructor (anyref.py:197-200), changeable later."""
        self.cfg.seg_token_idx = seg_token_idx
        if self.h is None:
            return
        lo, hi = self.cfg.seg_range()
        self._check(self.lib.anyref_set_seg_range(self.h, lo, hi), "set_seg_range")

    def set_overlap(self, on: bool):
        """SAM encoder on a second stream under the LLM decode (default) or everything on one stream."""
        self._check(self.lib.anyref_set_overlap(self.h, int(on)), "set_overlap")

    def set_early_tail(self, on: bool):
        """Masks of generated [SEG]s decoded on the side stream while the greedy loop goes on (default; batch 1)."""
        self._check(self.lib.anyref_set_early_tail(self.h, int(on)), "set_early_tail")

    @property
    def early_masks_done(self) -> int:
        """masks the last `generate` / session `generate` decoded early, on the side stream (0: the path did not run)"""
        return int(self.lib.anyref_early_masks_done(self.h))

    def set_rephrase_paths(self, on: bool):
        """`rephrase_weight > 0` on the fast paths (default off): the rephrase term of every image by one fused
        launch pair, and with it early [SEG] masks, drafts and image sessions under rephrasing.  Off: rephrasing runs its
        per-image chain after the loop, ignores drafts and is refused inside a session, as before the switch existed."""
        self._check(self.lib.anyref_set_rephrase_paths(self.h, int(on)), "set_rephrase_paths")

    def set_graphs(self, on: bool):
        """hipGraph replay of the greedy decode step (default) or eager launches."""
        self._check(self.lib.anyref_set_graphs(self.h, int(on)), "set_graphs")

    def set_side_share(self, wgs: int, steps: int = 0):
        """Workgroup cap of the SAM encoder's GEMM / attention launches while it co-runs with the decode loop (0: none),
        and the number of decode steps its blocks are spread over (0: keep)."""
        self._check(self.lib.anyref_set_side_share(self.h, int(wgs), int(steps)), "set_side_share")

    # ---- draft-verified greedy decode (anyref_set_draft) ----------------------------------------
    def set_draft_policy(self, policy: Optional[str]):
        """`"last"`: a `generate` call without `draft_ids` proposes, per row index, the tokens that row generated in the
        previous call with the same batch size -- the eval loops, whose answers are one of a few fixed templates, then have
        the answer checked in one pass over the weights instead of one per token.  `None` (default): no draft unless the
        caller passes one.  A draft never changes what is generated."""
        if policy not in (None, "last"):
            raise ValueError('draft policy is "last" or None')
        self._draft_policy = policy
        self._last_answers = None

    def set_draft(self, drafts):
        """One-shot proposal for the next `generate` (cleared by the next generate / forward whether used or not):
        a list of B token lists (empty / None: no draft for that row), or None to cancel."""
        if drafts is None:
            self._check(self.lib.anyref_set_draft(self.h, None, None, 0, 0), "set_draft")
            return
        rows = [[] if d is None else [int(v) for v in d] for d in drafts]
        B, K = len(rows), max(1, max(len(r) for r in rows))
        ids = torch.zeros(B, K, dtype=torch.long)
        for b, r in enumerate(rows):
            ids[b, : len(r)] = torch.tensor(r, dtype=torch.long)
        lens = torch.tensor([len(r) for r in rows], dtype=torch.int32)
        self._check(self.lib.anyref_set_draft(self.h, _ptr(ids), _ptr(lens), B, K), "set_draft")

    def draft_stats(self, B: int):
        """Of the last `generate`: dict(draft_offered i32 [B], draft_accepted i32 [B], decode_steps, verify_passes)."""
        off = torch.zeros(B, dtype=torch.int32)
        acc = torch.zeros(B, dtype=torch.int32)
        steps, passes = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.anyref_draft_stats(self.h, _ptr(off), _ptr(acc), B, C.byref(steps), C.byref(passes)),
                    "draft_stats")
        return dict(draft_offered=off, draft_accepted=acc, decode_steps=int(steps.value), verify_passes=int(passes.value))

    # ---- token scores (anyref_set_token_scores) ---------------------------------------------------
    def set_token_scores(self, on: bool):
        """Per-token confidence of everything generated (default off): with it on, every generated token of
        `generate`, `ImageSession.generate`, `SessionPool.generate` / `generate_many` carries its log-probability and its
        top-2 logit gap, computed on the device from the logits row that decided it (`last_token_scores`).  Off: nothing is
        launched or allocated for it.  What is generated is the same either way."""
        self._check(self.lib.anyref_set_token_scores(self.h, int(bool(on))), "set_token_scores")
        self._scores_on = bool(on)
        self._scores_call = self._scores_many = None

    def _generated(self, rows: int, max_new_tokens: int):
        """every generating call, after the library returned: whose scores `last_token_scores` reads"""
        self._scores_call = (int(rows), int(max_new_tokens))
        self._scores_many = None

    def _read_token_scores(self):
        if self._scores_call is None:
            return []
        B, cap = self._scores_call
        lp = torch.zeros(B, max(cap, 1), dtype=torch.float32)
        gap = torch.zeros(B, max(cap, 1), dtype=torch.float32)
        n = torch.zeros(B, dtype=torch.int32)
        self._check(self.lib.anyref_token_scores(self.h, B, max(cap, 1), _ptr(lp), _ptr(gap), _ptr(n)), "token_scores")
        return [dict(logprob=lp[b, : int(n[b])].clone(), gap=gap[b, : int(n[b])].clone()) for b in range(B)]

    def last_token_scores(self):
        """One entry per row of the last `generate`, `ImageSession.generate`, `SessionPool.generate` or `generate_many` call
        (there: per item, in the caller's item order): a dict of `logprob` and `gap`, CPU f32 tensors of length n_b aligned
        with the generated part of `output_ids[b]` -- logprob = x[id] - logsumexp(x), gap = x[id] - the greatest other logit
        (0 on a tie) of the f32 logits row x that decided the token (anyref_amd/scores.py).  RuntimeError while the switch
        is off."""
        if not self._scores_on:
            raise RuntimeError("last_token_scores: token scores are off (model.set_token_scores(True) before the call)")
        if self._scores_many is not None:
            return list(self._scores_many)
        return self._read_token_scores()

    # ---- mask reports (anyref_set_mask_reports) ----------------------------------------------------
    def set_mask_reports(self, on: bool, offset: float = 1.0, packed: bool = False):
        """What a caller wants to know about a mask without copying its f32 plane out (default off): with it
        on, every mask of `generate`, `forward`, `seg_tail`, `ImageSession.generate`, `SessionPool.generate` /
        `generate_many` is read once more on the device and leaves its area, its bounding box, SAM's stability score at
        `offset`, and a count of non-finite logits (`last_mask_reports`).  `packed=True` also keeps the binary mask, 32 pixels
        to a word, on the device: every such call then allocates sum_b max_seg * H_b * ceil(W_b / 32) words for it.  Off:
        nothing is launched or allocated.  What the calls return is the same either way."""
        self._check(self.lib.anyref_set_mask_reports(self.h, int(bool(on)), float(offset)), "set_mask_reports")
        self._reports_on = bool(on)
        self._reports_packed = bool(on) and bool(packed)
        self._reports_call = self._reports_many = None

    def _masks_begin(self, heights, widths):
        """every mask-producing call, right before the library is entered: the reports of the call before are gone, and with
        `packed` the buffer for this call's packed masks is armed (one-shot: the library takes it at its entry)"""
        self._reports_call = self._reports_many = None
        if not self._reports_on:
            return None
        buf = None
        if self._reports_packed:
            from .maskreport import packed_width
            words = sum(self.max_seg * int(h) * packed_width(w) for h, w in zip(heights, widths))
            buf = torch.empty(max(words, 1), device=self.device, dtype=torch.int32)
            self._check(self.lib.anyref_set_packed_masks(self.h, _ptr(buf), words), "set_packed_masks")
        return [int(h) for h in heights], [int(w) for w in widths], buf

    def _masks_made(self, pending):
        """... and after it returned: whose reports `last_mask_reports` reads"""
        self._reports_call = pending

    def _read_mask_reports(self):
        from .maskreport import packed_width, stability
        if self._reports_call is None:
            return []
        heights, widths, buf = self._reports_call
        B, cap = len(heights), max(self.max_seg, 1)
        n = torch.zeros(B, dtype=torch.int32)
        rec = torch.zeros(B, cap, 8, dtype=torch.int32)
        po = torch.zeros(B, dtype=torch.long)
        self._check(self.lib.anyref_mask_reports(self.h, B, cap, _ptr(n), _ptr(rec), _ptr(po)), "mask_reports")
        out = []
        for b in range(B):
            k = int(n[b])
            r = rec[b, :k].to(torch.long)
            words = heights[b] * packed_width(widths[b])
            out.append(dict(
                area=r[:, 0].clone(), area_hi=r[:, 1].clone(), area_lo=r[:, 2].clone(), nonfinite=r[:, 3].clone(),
                box=r[:, 4:8].clone(), stability=torch.from_numpy(stability(rec[b, :k].numpy())),
                packed=None if buf is None else buf[int(po[b]): int(po[b]) + k * words].view(k, heights[b], packed_width(widths[b]))))
        return out

    def last_mask_reports(self):
        """One entry per row of the last `generate`, `forward`, `seg_tail`, `ImageSession.generate`, `SessionPool.generate` or
        `generate_many` call (there: per item, in the caller's item order), for the n_b masks the library produced for the row
        (its `out_nseg`): a dict of `area`, `area_hi`, `area_lo`, `nonfinite` (int64 [n_b]), `box` (int64 [n_b, 4]: inclusive
        x0, y0, x1, y1; zeros for an empty mask), `stability` (f32 [n_b], NaN where area_lo is 0), all on the CPU, and
        `packed`: an int32 [n_b, H, ceil(W / 32)] view of that call's device buffer (`maskreport.unpack` / `maskreport.rle`
        read it), or None without `packed=True`.  The rule: anyref_amd/maskreport.py.  RuntimeError while the switch is off."""
        if not self._reports_on:
            raise RuntimeError("last_mask_reports: mask reports are off (model.set_mask_reports(True) before the call)")
        if self._reports_many is not None:
            return list(self._reports_many)
        return self._read_mask_reports()

    # ---- per-kernel timing for bench.py ------------------------------------------------------
    def profile_enable(self, on: bool, only_tag: Optional[str] = None, sample_every: int = 1):
        self._check(self.lib.anyref_profile_config(self.h, only_tag.encode() if only_tag else None, sample_every),
                    "profile_config")
        if on:  # what an empty event pair reads on this stream is taken off every bracket
            ov = C.c_double()
            self._check(self.lib.anyref_profile_calibrate(self.h, self._stream(), C.byref(ov)), "profile_calibrate")
            self.profile_overhead_us = ov.value
        self._check(self.lib.anyref_profile_enable(self.h, int(on)), "profile_enable")

    def profile_read(self):
        """-> {tag: dict(ms, count, flops, bytes)} of everything timed since profile_enable(True)."""
        torch.cuda.synchronize(self.device)
        self._check(self.lib.anyref_profile_collect(self.h), "profile_collect")
        out, i = {}, 0
        name = C.create_string_buffer(128)
        ms, cnt, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        while self.lib.anyref_profile_read(self.h, i, name, 128, C.byref(ms), C.byref(cnt), C.byref(fl),
                                           C.byref(by)) == 0:
            out[name.value.decode()] = dict(ms=ms.value, count=cnt.value, flops=fl.value, bytes=by.value)
            i += 1
        return out

    def stamps_enable(self, on: bool):
        """Kernel-side timestamps of the decode GEMVs (include/anyref_hip.h `anyref_stamps_*`): what bench.py's in-situ
        roofline reads -- production launch path (hipGraph replay, SAM encoder co-running), no event brackets."""
        torch.cuda.synchronize(self.device)
        self._check(self.lib.anyref_stamps_enable(self.h, int(on)), "stamps_enable")

    def stamps_read(self):
        """-> [dict(tag, t0_us, t1_us, bytes, epoch)] of every stamped launch since enable / the last read, by start time."""
        torch.cuda.synchronize(self.device)
        n = _lib._L()
        self._check(self.lib.anyref_stamps_dropped(self.h, C.byref(n)), "stamps_dropped")
        self.stamps_dropped = int(n.value)      # launches of this pass that went unstamped (record / epoch capacity): 0 or the rows lie
        self._check(self.lib.anyref_stamps_collect(self.h, C.byref(n)), "stamps_collect")
        name = C.create_string_buffer(128)
        t0, t1, by, ep = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        rows = []
        for i in range(n.value):
            if self.lib.anyref_stamps_read(self.h, i, name, 128, C.byref(t0), C.byref(t1), C.byref(by), C.byref(ep)) != 0:
                break
            a, b, c = C.c_double(), C.c_double(), C.c_double()
            self.lib.anyref_stamps_spread(self.h, i, C.byref(a), C.byref(b), C.byref(c))
            rows.append(dict(tag=name.value.decode(), t0_us=t0.value, t1_us=t1.value, bytes=by.value, epoch=ep.value,
                             start_spread_us=a.value, end_spread_us=b.value, wg_median_us=c.value))
        return rows

    def postprocess(self, low: torch.Tensor, resized_size, original_size) -> torch.Tensor:
        """`Sam.postprocess_masks` (sam.py:137-172) on low-res logits [n, 4g, 4g] -> [n, H, W]."""
        low = low.to(self.device, torch.float32).contiguous()
        n, lh, lw = low.shape
        out = torch.empty(n, int(original_size[0]), int(original_size[1]), device=self.device, dtype=torch.float32)
        if n:
            rc = self.lib.anyref_op_postprocess(self._stream(), _ptr(low), n, lh, lw, self.cfg.sam.img_size,
                                                int(resized_size[0]), int(resized_size[1]), int(original_size[0]),
                                                int(original_size[1]), _ptr(out))
            if rc != 0:
                raise RuntimeError("postprocess: " + self.lib.anyref_op_last_error().decode())
        return out

    # ---- helpers ---------------------------------------------------------------------------
    def _rows(self, input_ids: torch.Tensor, attention_masks: Optional[torch.Tensor], keep_out: Optional[list] = None,
              keep_in: Optional[list] = None):
        """-> (ids int64 host [B,Lmax] right-aligned rows, lens int32 [B]).

        `keep_out` receives the per-row index tensors that were kept; `keep_in` applies such a list instead of
        deriving one (labels must be cut exactly where their `input_ids` row was: a label row holds -100 / ids and
        never equals the pad id, so the pad rule below cannot be evaluated on it)."""
        ids = input_ids.detach().to("cpu", torch.long)
        if ids.dim() == 1:
            ids = ids[None]
        B, Lm = ids.shape
        rows = []
        pad = self.config.pad_token_id
        for b in range(B):
            r = ids[b]
            keep = torch.arange(Lm)
            if keep_in is not None:
                keep = keep_in[b]
            elif attention_masks is not None:
                keep = attention_masks[b].to("cpu").bool().nonzero().flatten()
            elif B > 1 and pad is not None:
                # the callers' batched path passes left-padded ids and NO mask (eval_referseg.py:124-137); the
                # collator's own mask is `input_ids.ne(pad_token_id)` (utils/coco_instance.py:142): strip the pad
                # runs at both ends of the row (pad = unk never opens or closes a prompt: BOS ... "ASSISTANT:")
                nz = (r != int(pad)).nonzero().flatten()
                keep = torch.arange(int(nz[0]), int(nz[-1]) + 1) if len(nz) else torch.arange(1)
            if keep_out is not None:
                keep_out.append(keep)
            rows.append(r[keep])
        lens = torch.tensor([len(r) for r in rows], dtype=torch.int32)
        out = torch.zeros(B, int(lens.max()), dtype=torch.long)
        for b, r in enumerate(rows):
            out[b, : len(r)] = r
        return out.contiguous(), lens

    def _extra_overlapped(self, ids, lens, audios, ref_feats):
        """`_extra` with the audio trunk + projector (launch-bound: ~1.3 ms of small kernels) on a stream of their own: the
        next C call waits for them only at the splice, so they run beside the CLIP tower instead of in front of it
        (anyref_set_extra_event).  Same kernels, same results."""
        # (HIP trunk inside the handle only: C4 41.1 -> 40.4 ms per image; the PyTorch-ROCm module's ~3 ms of host-side launches sit in
        #  front of the C call whatever stream they go to: 42.2 vs 42.5 ms)
        if audios is None or self.cfg.audio_trunk is None or self.device.type != "cuda" or os.environ.get("ANYREF_AUDIO_OVERLAP", "1") == "0":
            return self._extra(ids, lens, audios, ref_feats)
        main = torch.cuda.current_stream(self.device)
        if getattr(self, "_audio_stream", None) is None:
            self._audio_stream = torch.cuda.Stream(self.device)
            self._audio_event = torch.cuda.Event()
        side = self._audio_stream
        side.wait_stream(main)                      # the mel clips / features the caller queued on its stream
        with torch.cuda.stream(side):
            out = self._extra(ids, lens, audios, ref_feats)
            self._audio_event.record(side)
        if out[0] is not None:
            out[0].record_stream(main)
        self._check(self.lib.anyref_set_extra_event(self.h, C.c_void_p(self._audio_event.cuda_event)), "set_extra_event")
        return out

    def _extra(self, ids: torch.Tensor, lens, audios, ref_feats):
        """Projected audio / reference features -> (extra_embeds dev [n,H], slots host [n,2])."""
        embeds, slots = [], []
        B = ids.shape[0]
        if audios is not None:
            for b in range(B):
                a = audios[b] if isinstance(audios, (list, tuple)) else audios[b:b + 1]
                if a is None:
                    continue
                if a.dim() >= 4:     # raw mel clips [1,3,1,128,204] -> ImageBind embedding [3,1024]
                    if self.cfg.audio_trunk is not None:          # trunk inside the handle (HIP, f-4)
                        a = self.audio_encode(a)
                    elif self.audio_encoder is not None:           # PyTorch-ROCm module (north_star's default)
                        _, emb = self.audio_encoder.get_audio_feature(a.to(self.device).float())
                        a = emb[0]
                    else:
                        raise RuntimeError("raw audio given but neither a HIP trunk (cfg.audio_trunk + model.audio_encoder.* "
                                           "weights) nor an audio_encoder module (anyref_amd.audio) is attached")
                a = a.to(self.device, torch.float32).reshape(-1, self.cfg.audio_dim).contiguous()
                out = torch.empty(a.shape[0], self.cfg.llm.dim, device=self.device, dtype=torch.float32)
                self._check(self.lib.anyref_project_audio(self.h, self._stream(), _ptr(a), a.shape[0], _ptr(out)),
                            "project_audio")
                pos = (ids[b, : lens[b]] == AUDIO_REF_INDEX).nonzero().flatten().tolist()
                if len(pos) != out.shape[0]:
                    raise ValueError(f"row {b}: {len(pos)} audio placeholders but {out.shape[0]} audio features")
                embeds.append(out)
                slots += [(b, p) for p in pos]
        if ref_feats is not None:
            for b in range(B):
                r = ref_feats[b]
                if r is None:
                    continue
                r = r.to(self.device, torch.float32).reshape(-1, self.cfg.llm.dim).contiguous()
                pos = (ids[b, : lens[b]] == IMG_REF_INDEX).nonzero().flatten().tolist()
                if len(pos) != r.shape[0]:
                    raise ValueError(f"row {b}: {len(pos)} image-ref placeholders but {r.shape[0]} features")
                embeds.append(r)
                slots += [(b, p) for p in pos]
        if not embeds:
            return None, None, 0
        e = torch.cat(embeds, 0).contiguous()
        s = torch.tensor(slots, dtype=torch.int32).contiguous()
        return e, s, e.shape[0]

    def _ref_features(self, ref_images, B: int):
        """`ref_images` branch of generate (anyref.py:681-702) / forward (:319-339): every reference image goes
        through `encode_images` (a second CLIP pass) and ends as IMG_REF_NUM rows that replace the prompt's
        `<img_ref>` placeholders.  The reference pools a TENSOR batch 256 -> 16 -> 4 in the glue (:695-700) but hands
        LIST items to the absent llava layer unpooled (:691-692); this backend's reading of that layer (INFERRED,
        documented in DESIGN.md) pools them the way `model_forward_new` does (:335-338), so both forms take the
        same kernel (`anyref_op_pool_ref_tokens`).  1-D items are RoI coordinates (:688-689): need the llava layer."""
        if ref_images is None:
            return None
        from .config import IMG_REF_NUM
        if isinstance(ref_images, (list, tuple)):
            items = list(ref_images)
        else:
            if ref_images.dim() != 4 or ref_images.shape[0] != B:          # anyref.py:695,701-702
                raise NotImplementedError("a ref_images tensor must be [batch, 3, S, S]")
            items = list(ref_images)
        feats = []
        for r in items:
            if r is None:
                feats.append(None)
                continue
            if r.dim() == 1:
                raise NotImplementedError("RoI-coordinate reference (anyref.py:688-689) needs the absent llava layer")
            f = self.encode_images(r[None].float())                      # [1, 256, H]
            out = torch.empty(1, IMG_REF_NUM, f.shape[2], device=self.device, dtype=torch.float32)
            rc = self.lib.anyref_op_pool_ref_tokens(self._stream(), _ptr(f), 1, f.shape[1], f.shape[2], IMG_REF_NUM, _ptr(out))
            if rc != 0:
                raise RuntimeError("pool_ref_tokens: " + self.lib.anyref_op_last_error().decode())
            feats.append(out[0])
        return feats

    # ---- stage calls (used by tests and by callers that want the pieces) -------------------
    def encode_images(self, clip_images: torch.Tensor, return_clip: bool = False):
        x = clip_images.to(self.device, torch.float32).contiguous()
        B = x.shape[0]
        out = torch.empty(B, self.n_img, self.cfg.llm.dim, device=self.device, dtype=torch.float32)
        cf = torch.empty(B, self.n_img, self.cfg.clip.dim, device=self.device, dtype=torch.float32) if return_clip else None
        self._check(self.lib.anyref_encode_images(self.h, self._stream(), _ptr(x), B, _ptr(out), _ptr(cf)),
                    "encode_images")
        return (out, cf) if return_clip else out

    def audio_encode(self, mel: torch.Tensor) -> torch.Tensor:
        """`get_audio_feature(...)[1]` (imagebind_model.py:477-511) in HIP: mel [..., 1, mel_bins, target_len] (any
        leading clip / batch dims) -> embedding [n_clips, audio_dim], L2-normalised x logit scale."""
        at = self.cfg.audio_trunk
        if at is None:
            raise RuntimeError("the handle was created without an audio trunk (cfg.audio_trunk is None)")
        x = mel.to(self.device, torch.float32).reshape(-1, 1, at.mel_bins, at.target_len).contiguous()
        out = torch.empty(x.shape[0], self.cfg.audio_dim, device=self.device, dtype=torch.float32)
        self._check(self.lib.anyref_audio_encode(self.h, self._stream(), _ptr(x), x.shape[0], _ptr(out)), "audio_encode")
        return out

    def sam_encode(self, sam_images: torch.Tensor) -> torch.Tensor:
        """-> [B, 256, g, g] (the reference's NCHW layout)."""
        x = sam_images.to(self.device, torch.float32).contiguous()
        B, g = x.shape[0], self.cfg.sam.grid
        out = torch.empty(B, g * g, self.cfg.sam.out_chans, device=self.device, dtype=torch.float32)
        self._check(self.lib.anyref_sam_encode(self.h, self._stream(), _ptr(x), B, _ptr(out)), "sam_encode")
        return out.view(B, g, g, -1).permute(0, 3, 1, 2)

    def mask_decode(self, image_embedding: torch.Tensor, pred_embeddings: Optional[torch.Tensor], resized_size=None,
                    original_size=None, points=None, point_labels=None, boxes=None, mask_input=None,
                    multimask_output: bool = False):
        """image_embedding [256,g,g] or [1,256,g,g]; pred_embeddings [n,256] ->
        dict(masks4 [n,4,4g,4g], iou [n,4], masks [n,H,W] if sizes given).

        With any of `points` [n,P,2] + `point_labels` [n,P], `boxes` [n,4], `mask_input` [n,4g,4g], `multimask_output`, or
        with `pred_embeddings=None` (a pure SAM prompt): the prompted path (`set_spatial_prompts` first).  Coordinates are in
        the SAM input frame, as for the reference's `predict_torch`.  It adds `low_res` [n,k,4g,4g] and `best` [n] to the
        dict; with `multimask_output`, `masks` is [n,3,H,W] (mask tokens 1..3)."""
        if pred_embeddings is None or multimask_output or any(a is not None for a in (points, point_labels, boxes, mask_input)):
            return self._mask_decode_prompted(image_embedding, pred_embeddings, resized_size, original_size, points,
                                              point_labels, boxes, mask_input, multimask_output)
        g, Cc = self.cfg.sam.grid, self.cfg.sam.out_chans
        e = image_embedding.reshape(Cc, g * g).t().to(self.device, torch.float32).contiguous()
        p = pred_embeddings.to(self.device, torch.float32).reshape(-1, self.cfg.out_dim).contiguous()
        n, nt = p.shape[0], self.cfg.sam.num_mask_tokens
        m4 = torch.empty(n, nt, 4 * g, 4 * g, device=self.device, dtype=torch.float32)
        iou = torch.empty(n, nt, device=self.device, dtype=torch.float32)
        out = rs = os_ = None
        if original_size is not None:
            out = torch.empty(n, int(original_size[0]), int(original_size[1]), device=self.device, dtype=torch.float32)
            rs = (C.c_int32 * 2)(int(resized_size[0]), int(resized_size[1]))
            os_ = (C.c_int32 * 2)(int(original_size[0]), int(original_size[1]))
        self._check(self.lib.anyref_mask_decode(self.h, self._stream(), _ptr(e), _ptr(p), n, _ptr(m4), _ptr(iou),
                                                rs, os_, _ptr(out)), "mask_decode")
        return dict(masks4=m4, iou=iou, masks=out)

    # ---- SAM spatial prompts beside [SEG] -----------------------------------
    def set_spatial_prompts(self, max_points: int = 8):
        """Reserve the prompted decoder path (`anyref_prompt_reserve`): points, boxes and low-res masks beside the [SEG]
        embedding in `mask_decode(...)` and `refine(...)`.  Needs the spatial weights of SAM's prompt encoder in the state
        dict (`anyref_amd.prompts.SPATIAL_NAMES`).  0 frees the workspaces.  While reserved, the generating calls keep their
        low-res logits for `refine(..., mask_input=True)`."""
        self._check(self.lib.anyref_prompt_reserve(self.h, int(max_points)), "prompt_reserve")
        self._sp_max = int(max_points)
        self._refine_ctx = None

    def _spatial(self, n, points, labels, boxes, mask_input, multimask):
        """-> (anyref_spatial_prompts, the device tensors it points to)"""
        L = 4 * self.cfg.sam.grid
        sp, keep = _lib.SpatialPrompts(), []

        def dev(t, dtype, shape):
            t = torch.as_tensor(t).to(self.device, dtype).reshape(shape).contiguous()
            keep.append(t)
            return t.data_ptr()
        if (points is None) != (labels is None):
            raise ValueError("points and point labels come together")
        if points is not None:
            lab = torch.as_tensor(labels).reshape(n, -1)
            if not bool(((lab == -1) | (lab == 0) | (lab == 1)).all()):
                raise ValueError("point labels are 1 (foreground), 0 (background) or -1 (not a point)")
            sp.n_points = lab.shape[1]
            sp.points, sp.labels = dev(points, torch.float32, (n, sp.n_points, 2)), dev(lab, torch.int32, (n, sp.n_points))
        if boxes is not None:
            sp.boxes = dev(boxes, torch.float32, (n, 4))
        if mask_input is not None:
            sp.mask_input = dev(mask_input, torch.float32, (n, L, L))
        sp.multimask = int(bool(multimask))
        return sp, keep

    def _mask_decode_prompted(self, image_embedding, pred_embeddings, resized_size, original_size, points, point_labels, boxes,
                              mask_input, multimask_output):
        g, Cc, L = self.cfg.sam.grid, self.cfg.sam.out_chans, 4 * self.cfg.sam.grid
        e = image_embedding.reshape(Cc, g * g).t().to(self.device, torch.float32).contiguous()
        p = None if pred_embeddings is None else \
            pred_embeddings.to(self.device, torch.float32).reshape(-1, self.cfg.out_dim).contiguous()
        if p is not None:                       # the prompt count, as the reference's _get_batch_size finds it
            n = p.shape[0]
        elif points is not None:
            n = torch.as_tensor(points).reshape(-1, torch.as_tensor(point_labels).shape[-1], 2).shape[0]
        elif boxes is not None:
            n = torch.as_tensor(boxes).reshape(-1, 4).shape[0]
        else:
            n = 1 if mask_input is None else torch.as_tensor(mask_input).reshape(-1, L, L).shape[0]
        nt, k = self.cfg.sam.num_mask_tokens, 3 if multimask_output else 1
        sp, keep = self._spatial(n, points, point_labels, boxes, mask_input, multimask_output)
        m4 = torch.empty(n, nt, L, L, device=self.device, dtype=torch.float32)
        iou = torch.empty(n, nt, device=self.device, dtype=torch.float32)
        out = rs = os_ = None
        if original_size is not None:
            out = torch.empty(n, k, int(original_size[0]), int(original_size[1]), device=self.device, dtype=torch.float32)
            rs = (C.c_int32 * 2)(int(resized_size[0]), int(resized_size[1]))
            os_ = (C.c_int32 * 2)(int(original_size[0]), int(original_size[1]))
        self._check(self.lib.anyref_mask_decode_prompted(self.h, self._stream(), _ptr(e), _ptr(p), n, C.byref(sp), _ptr(m4),
                                                         _ptr(iou), rs, os_, _ptr(out)), "mask_decode_prompted")
        from .prompts import pick
        tokens, best = pick(iou, multimask_output)
        if out is not None and not multimask_output:
            out = out[:, 0]
        return dict(masks4=m4, iou=iou, masks=out, low_res=m4[:, tokens], best=best)

    def refine_embedding(self, row: int, seg: int) -> torch.Tensor:
        """the [SEG] prompt embedding [out_dim] that `refine(row, seg)` starts from (`anyref_refine_embedding`)"""
        out = torch.empty(self.cfg.out_dim, device=self.device, dtype=torch.float32)
        self._check(self.lib.anyref_refine_embedding(self.h, self._stream(), int(row), int(seg), _ptr(out)), "refine_embedding")
        return out

    def _refine_keep(self, out_low, resized, height, width):
        """after a generating call: what `refine` needs of it on the host"""
        self._refine_ctx = dict(low=out_low, resized=[(int(a), int(b)) for a, b in resized],
                                orig=[(int(h), int(w)) for h, w in zip(height, width)]) if self._sp_max else None

    @torch.no_grad()
    def refine(self, row: int, seg: int, points=None, labels=None, box=None, mask_input=None, multimask_output: bool = False):
        """Decode mask `seg` of row `row` of the last `generate` / session / pooled call again, with spatial prompts ADDED to
        that [SEG]'s own embedding (`anyref_refine_masks`).  Coordinates are in ORIGINAL image pixels, as for the reference's
        `SamPredictor.predict`: points [P, 2] (x, y) with labels [P] in {1, 0, -1}, box [4] (x0 y0 x1 y1).  `mask_input`: low-res
        logits [4g, 4g], or True for the ones this mask had.  -> dict(masks [k, H, W], low_res [k, 4g, 4g], iou [k], best),
        k = 3 with `multimask_output` (mask tokens 1..3, best = argmax of their predicted IoU), else 1."""
        from .prompts import pick, to_input_frame
        ctx = getattr(self, "_refine_ctx", None)
        if not self._sp_max:
            raise RuntimeError("refine: spatial prompts are not reserved (model.set_spatial_prompts() first)")
        if ctx is None or not (0 <= int(row) < len(ctx["orig"])):
            raise RuntimeError("refine: row outside the last generating call (or none since set_spatial_prompts)")
        row, seg = int(row), int(seg)
        rhw, ohw = ctx["resized"][row], ctx["orig"][row]
        if points is not None:
            points = to_input_frame(torch.as_tensor(points, dtype=torch.float64).reshape(-1, 2), ohw, rhw)
        if box is not None:
            box = to_input_frame(torch.as_tensor(box, dtype=torch.float64).reshape(2, 2), ohw, rhw).reshape(4)
        if mask_input is True:
            if not (0 <= seg < ctx["low"].shape[1]):
                raise RuntimeError("refine: seg outside the row's masks of the last call")
            mask_input = ctx["low"][row, seg]
        L, nt, k = 4 * self.cfg.sam.grid, self.cfg.sam.num_mask_tokens, 3 if multimask_output else 1
        sp, keep = self._spatial(1, points, labels, box, mask_input, multimask_output)
        low = torch.empty(k, L, L, device=self.device, dtype=torch.float32)
        iou = torch.empty(nt, device=self.device, dtype=torch.float32)
        out = torch.empty(k, ohw[0], ohw[1], device=self.device, dtype=torch.float32)
        self._check(self.lib.anyref_refine_masks(self.h, self._stream(), row, seg, C.byref(sp), _ptr(low), _ptr(iou), _ptr(out)),
                    "refine_masks")
        tokens, best = pick(iou, multimask_output)
        return dict(masks=out, low_res=low, iou=iou[tokens], best=int(best))

    def llm_forward(self, embeds: torch.Tensor, lens: Optional[Sequence[int]] = None, want_logits: bool = False,
                    attn_q: Optional[Sequence[int]] = None):
        x = embeds.to(self.device, torch.float32).contiguous()
        B, S, H = x.shape
        ln = (C.c_int32 * B)(*([S] * B if lens is None else [int(v) for v in lens]))
        hidden = torch.empty(B, S, H, device=self.device, dtype=torch.float32)
        logits = torch.empty(B, S, self.cfg.llm.vocab, device=self.device, dtype=torch.float32) if want_logits else None
        aq = ar = None
        if attn_q is not None:
            aq = (C.c_int32 * B)(*[int(v) for v in attn_q])
            ar = torch.zeros(B, S, device=self.device, dtype=torch.float32)
        self._check(self.lib.anyref_llm_forward(self.h, self._stream(), _ptr(x), ln, B, S, _ptr(hidden), _ptr(logits),
                                                aq, _ptr(ar)), "llm_forward")
        return dict(hidden=hidden, logits=logits, attn_row=ar)

    def llm_extend(self, embeds: torch.Tensor, pos0: Sequence[int], lens: Optional[Sequence[int]] = None,
                   want_logits: bool = False):
        """`anyref_llm_extend`: n new rows per sequence behind the KV cache the previous `llm_forward` / `llm_extend` left,
        row i of sequence b at position pos0[b] + i.  -> dict(hidden [B,n,H], logits [B,n,vocab] | None); hidden rows at and
        past lens[b] are NaN (never written), logits rows there are undefined."""
        x = embeds.to(self.device, torch.float32).contiguous()
        B, n, H = x.shape
        p0 = (C.c_int32 * B)(*[int(v) for v in pos0])
        ln = (C.c_int32 * B)(*([n] * B if lens is None else [int(v) for v in lens]))
        hidden = torch.full((B, n, H), float("nan"), device=self.device, dtype=torch.float32)
        logits = torch.empty(B, n, self.cfg.llm.vocab, device=self.device, dtype=torch.float32) if want_logits else None
        self._check(self.lib.anyref_llm_extend(self.h, self._stream(), _ptr(x), p0, ln, B, n, _ptr(hidden), _ptr(logits)),
                    "llm_extend")
        return dict(hidden=hidden, logits=logits)

    def seg_tail(self, sam_images, ids, ids_lens, ref_pos, hidden, attn_mean, sam_resized_sizes, height, width,
                 teacher: bool = False):
        """The glue alone (anyref.py:718-822 / :273-282,:356-430) on caller-provided LLM outputs:
        ids [B,L] (`outputs.sequences` or, teacher=True, `input_ids`), hidden [B,rows,H] = `hidden_states[-1]`,
        attn_mean [B,rows,rows] head-mean `attentions[-1]` (only with rephrase_weight > 0), ref_pos [B] = prompt
        length (generate) or `where(labels > 0)[0][0]` (forward).  -> (pred_masks list | None, nseg)."""
        ids = ids.detach().to("cpu", torch.long).contiguous()
        B, Lmax = ids.shape
        lens = torch.tensor([int(v) for v in ids_lens], dtype=torch.int32)
        rp = None if ref_pos is None else torch.tensor([int(v) for v in ref_pos], dtype=torch.int32)
        hid = hidden.to(self.device, torch.float32).contiguous()
        att = None if attn_mean is None else attn_mean.to(self.device, torch.float32).contiguous()
        sam = sam_images.to(self.device, torch.float32).contiguous()
        height, width = [int(h) for h in height], [int(w) for w in width]
        rs = torch.tensor([[int(a), int(b)] for a, b in sam_resized_sizes], dtype=torch.int32).contiguous()
        os_ = torch.tensor([[h, w] for h, w in zip(height, width)], dtype=torch.int32).contiguous()
        nseg = torch.zeros(B, dtype=torch.int32)
        offs = torch.zeros(B, dtype=torch.long)
        cap = sum(self.max_seg * h * w for h, w in zip(height, width))
        out_masks = torch.empty(cap, device=self.device, dtype=torch.float32)
        pending = self._masks_begin(height, width)
        self._check(self.lib.anyref_seg_tail(self.h, self._stream(), _ptr(sam), _ptr(ids), _ptr(lens), _ptr(rp), B, Lmax,
                                             int(teacher), _ptr(hid), hid.shape[1], _ptr(att), _ptr(rs), _ptr(os_),
                                             _ptr(nseg), _ptr(out_masks), cap, _ptr(offs), None), "seg_tail")
        self._masks_made(pending)
        if int(nseg.sum()) == 0:
            return None, nseg
        return [out_masks[int(offs[b]): int(offs[b]) + int(nseg[b]) * height[b] * width[b]].view(int(nseg[b]), height[b], width[b])
                for b in range(B)], nseg

    # ---- the reference surface -------------------------------------------------------------
    @torch.no_grad()
    def generate(self, clip_images, input_ids, sam_images, sam_resized_sizes, height, width, audios=None,
                 ref_images=None, output_hidden_states=True, return_dict_in_generate=True, max_new_tokens=128,
                 attention_masks=None, _return_extras: bool = False, draft_ids=None):
        """`AnyRefForCausalLM.generate` (model/anyref.py:647-822).

        `draft_ids` (trailing keyword, not in the reference): a proposed answer per row -- the generated tokens from the
        first one on -- as a list of B 1-D tensors / lists (None entries allowed) or a [B, K] tensor whose rows end at the
        first negative id.  The backend checks it in one pass over the weights and falls back to the one-token loop where it
        stops matching; the output is the same greedy decode either way (`set_draft_policy`)."""
        ids, lens = self._rows(input_ids, attention_masks)
        B, Lmax = ids.shape
        if B > self.max_batch:
            raise ValueError(f"batch {B} > max_batch {self.max_batch} the handle was created for")
        drafts = None
        if draft_ids is not None:
            from .draft import normalize_drafts
            drafts = normalize_drafts(draft_ids, B)
        elif self._draft_policy == "last" and self._last_answers is not None and len(self._last_answers) == B:
            drafts = self._last_answers
        clip = clip_images.to(self.device, torch.float32).contiguous()
        sam = sam_images.to(self.device, torch.float32).contiguous()
        extra, slots, n_extra = self._extra_overlapped(ids, lens, audios, self._ref_features(ref_images, B))
        height = [int(h) for h in height]
        width = [int(w) for w in width]
        rs = torch.tensor([[int(a), int(b)] for a, b in sam_resized_sizes], dtype=torch.int32).contiguous()
        os_ = torch.tensor([[h, w] for h, w in zip(height, width)], dtype=torch.int32).contiguous()
        Lout = Lmax + max_new_tokens
        out_ids = torch.zeros(B, Lout, dtype=torch.long)
        out_lens = torch.zeros(B, dtype=torch.int32)
        out_nseg = torch.zeros(B, dtype=torch.int32)
        offs = torch.zeros(B, dtype=torch.long)
        cap = sum(self.max_seg * h * w for h, w in zip(height, width))
        out_masks = torch.empty(cap, device=self.device, dtype=torch.float32)
        out_low = hid = None
        if _return_extras or self._sp_max:   # low-res logits (what a DP driver all-gathers; what refine(mask_input=True) feeds back)
            L = 4 * self.cfg.sam.grid
            out_low = torch.zeros(B, self.max_seg, L, L, device=self.device, dtype=torch.float32)
            if _return_extras and _return_extras != "low":   # ... and, unless "low", the hidden states
                hid = torch.empty(B, self.cfg.llm.max_seq, self.cfg.llm.dim, device=self.device, dtype=torch.float32)
        eos = self.config.eos_token_id if self.config.eos_token_id is not None else -1
        if drafts is not None and any(drafts):
            self.set_draft(drafts)
        pending = self._masks_begin(height, width)
        self._check(self.lib.anyref_generate(
            self.h, self._stream(), _ptr(clip), _ptr(sam), _ptr(ids), _ptr(lens), B, Lmax, _ptr(extra),
            _ptr(slots), n_extra, _ptr(rs), _ptr(os_), int(max_new_tokens), int(eos), _ptr(out_ids), _ptr(out_lens),
            _ptr(out_nseg), _ptr(out_masks), cap, _ptr(offs), _ptr(out_low), _ptr(hid)), "generate")
        self._generated(B, max_new_tokens)
        self._masks_made(pending)
        self._refine_keep(out_low, sam_resized_sizes, height, width)
        if self._draft_policy == "last":
            self._last_answers = [out_ids[b, int(lens[b]): int(out_lens[b])].tolist() for b in range(B)]
        res = self._result(out_ids, out_lens, out_nseg, offs, out_masks, height, width)
        if _return_extras:
            return res, dict(out_lens=out_lens, nseg=out_nseg, low_res=out_low, hidden=hid, **self.draft_stats(B))
        return res

    def _result(self, out_ids, out_lens, out_nseg, offs, out_masks, height, width, per_row=False):
        """what `generate` returns, from the buffers anyref_generate / anyref_session_generate filled.  per_row (a session: its
        rows are independent queries, each what a one-row plain call returns): the reference's "fewer [SEG]s than samples"
        rule under rephrasing is a property of ONE batched call and is not applied across the rows -- a row without a [SEG]
        gets an empty [0, h, w] mask tensor, the other rows keep their masks"""
        B = out_ids.shape[0]
        # HF pads finished rows with pad_token_id
        full = torch.full((B, int(out_lens.max())), int(self.config.pad_token_id or 0), dtype=torch.long)
        for b in range(B):
            full[b, : out_lens[b]] = out_ids[b, : out_lens[b]]
        output_ids = full.to(self.device)
        total = int(out_nseg.sum())
        if total == 0:                                    # anyref.py:729-730
            res = (output_ids, None, (None, None, None))
        elif self.cfg.rephrase_weight > 0 and total < B and not per_row:  # (3-tuple in the reference too)
            # anyref.py:739-744,763-765: with rephrase on, the reference indexes the flattened [SEG] list by sample; fewer
            # [SEG] tokens than samples is its IndexError -> `no_mask` path: one all-zero [1, height[0], width[0]] mask per
            # sample (the same tensor object bs times), whatever the other rows produced
            z = torch.zeros((1, height[0], width[0]), device=self.device, dtype=torch.float32)
            res = (output_ids, [z] * B, (None, None, None))
        else:
            pred_masks = []
            for b in range(B):
                n, h, w = int(out_nseg[b]), height[b], width[b]
                o = int(offs[b])
                pred_masks.append(out_masks[o: o + n * h * w].view(n, h, w))
            res = (output_ids, pred_masks, (None, None, None))
        if self.success_arity == 2 and res[1] is not None and not (self.cfg.rephrase_weight > 0 and total < B and not per_row):
            res = res[:2]                                 # the reference's own success path (anyref.py:822): any [SEG], no `no_mask`
        return res

    def image_session(self, clip_image, sam_image, sam_resized_size, height, width, prefix_ids) -> "ImageSession":
        """Encode one image once and answer many queries behind its cache (`anyref_session_open`): the CLIP
        tower, the SAM encoder and the prefill of `prefix_ids` -- the start every prompt about this image shares, up to and
        including the image placeholder -- run here; `sess.generate(...)` then costs the suffix and the answer only.

            with model.image_session(clip, sam, resized, h, w, ids[: image_pos + 1]) as sess:
                for ids in prompts_about_this_image:
                    out_ids, masks, _ = sess.generate(ids, max_new_tokens=...)

        clip_image [3, S, S] or [1, 3, S, S]; sam_resized_size (h, w) and height / width of the one image (one-element lists as
        `generate` takes them are accepted).  One session per model: opening another replaces it, and any other call that runs
        the model (`generate`, `forward`, `llm_forward`, `encode_images`, ...) ends it."""
        return ImageSession(self, clip_image, sam_image, sam_resized_size, height, width, prefix_ids)

    def session_pool(self, slots: int, max_prefix_rows: Optional[int] = None) -> "SessionPool":
        """Keep up to `slots` images resident and ask about any of them, several per call (`anyref_session_pool_reserve`,
        DESIGN.md §8.11): a stream that interleaves images pays one open per NEW image instead of one per switch, questions about
        different images share a call, and plain calls in between (`generate`, `forward`, ...) do not lose the images.

            pool = model.session_pool(8)
            ps = pool.get(image_id) or pool.open(image_id, clip, sam, resized, h, w, ids[: image_pos + 1])
            out_ids, masks, _ = pool.generate([ps_a, ps_b, ps_a], prompts, max_new_tokens=...)

        A slot reserves `max_prefix_rows` prefix rows of every layer's K and V (default: llm_max_seq - 2, capped at the image rows
        + 128 prompt ids -- `session.default_max_prefix_rows`); at LLaMA-7B with 16-bit caches about 0.52 MB per row and slot.
        One pool per model: a second call re-reserves, which the library allows only while every slot is empty, and closes
        the pool handed out before.  Switching
        an adapter (`set_adapter`) ends every slot in the library ("slot N lost: ended by ..." at the C entry); the pool then
        forgets its sessions as well: `pool.get(key)` returns None, a session object handed out before raises on use, and the
        images are opened again."""
        pool = SessionPool(self, slots, max_prefix_rows)   # (raises, and changes nothing, if the library refuses to re-reserve)
        if self._session_pool is not None:           # the pool before it shares the library's slots: it is closed
            self._session_pool._forget_all()
            self._session_pool.closed = True
        self._session_pool = pool
        return pool

    def forward(self, **kwargs):
        """`AnyRefForCausalLM.forward` (anyref.py:233-237): dispatch as the reference does."""
        if "past_key_values" in kwargs:
            raise NotImplementedError("plain LM forward with past_key_values is handled inside the HIP decode loop")
        return self.model_forward_new(**kwargs)

    __call__ = forward

    @torch.no_grad()
    def model_forward_new(self, clip_images, sam_images, input_ids, labels, attention_masks, sam_resized_sizes,
                          gt_masks, height, width, audios=None, ref_images=None, _return_extras: bool = False,
                          **kwargs):
        """Teacher-forced `model_forward_new` (anyref.py:239-466), inference arithmetic on the GPU,
        losses (`anyref.py:19-68,432-450`) evaluated with torch on the returned logits."""
        keeps: list = []
        ids, lens = self._rows(input_ids, attention_masks, keep_out=keeps)
        B, Lmax = ids.shape
        lab_rows, _ = self._rows(labels, None, keep_in=keeps)   # the same positions as the ids, whatever chose them
        clip = clip_images.to(self.device, torch.float32).contiguous()
        sam = sam_images.to(self.device, torch.float32).contiguous()
        extra, slots, n_extra = self._extra(ids, lens, audios, self._ref_features(ref_images, B))
        height = [int(h) for h in height]
        width = [int(w) for w in width]
        rs = torch.tensor([[int(a), int(b)] for a, b in sam_resized_sizes], dtype=torch.int32).contiguous()
        os_ = torch.tensor([[h, w] for h, w in zip(height, width)], dtype=torch.int32).contiguous()
        out_nseg = torch.zeros(B, dtype=torch.int32)
        offs = torch.zeros(B, dtype=torch.long)
        cap = sum(self.max_seg * h * w for h, w in zip(height, width))
        out_masks = torch.empty(cap, device=self.device, dtype=torch.float32)
        reph = torch.zeros(B, dtype=torch.int32)
        for b in range(B):
            pos = (lab_rows[b, : lens[b]] > 0).nonzero().flatten()
            reph[b] = int(pos[0]) if len(pos) else 0
        has_img = [(ids[b, : lens[b]] == IMAGE_TOKEN_INDEX).any().item() for b in range(B)]
        Sp = max(int(lens[b]) + (self.n_img - 1 if has_img[b] else 0) for b in range(B))
        logits = torch.empty(B, Sp, self.cfg.llm.vocab, device=self.device, dtype=torch.float32)
        hid = torch.empty(B, self.cfg.llm.max_seq, self.cfg.llm.dim, device=self.device,
                          dtype=torch.float32) if _return_extras else None
        pending = self._masks_begin(height, width)
        self._check(self.lib.anyref_forward_teacher(
            self.h, self._stream(), _ptr(clip), _ptr(sam), _ptr(ids), _ptr(lens), B, Lmax, _ptr(extra), _ptr(slots),
            n_extra, _ptr(reph), _ptr(rs), _ptr(os_), _ptr(out_nseg), _ptr(out_masks), cap, _ptr(offs), None,
            _ptr(hid), _ptr(logits)), "forward_teacher")
        self._masks_made(pending)
        # LM loss (HF shift-by-one CE; the image span carries IGNORE labels)
        num, den = torch.zeros((), device=self.device), 0
        for b in range(B):
            lab = lab_rows[b, : lens[b]]
            if has_img[b]:
                ip = int((ids[b, : lens[b]] == IMAGE_TOKEN_INDEX).nonzero()[0])
                lab = torch.cat([lab[:ip], torch.full((self.n_img,), -100, dtype=torch.long), lab[ip + 1:]])
            lab = lab.to(self.device)
            valid = lab[1:] != -100
            if valid.any():
                lg = logits[b, : lab.shape[0] - 1][valid]
                num = num + F.cross_entropy(lg, lab[1:][valid], reduction="sum")
                den += int(valid.sum())
        lm_loss = num / max(den, 1)
        if int(out_nseg.sum()) == 0:                      # anyref.py:356-365
            return {"loss": lm_loss, "lm_loss": lm_loss}
        pred_masks = []
        for b in range(B):
            n, h, w = int(out_nseg[b]), height[b], width[b]
            o = int(offs[b])
            pred_masks.append(out_masks[o: o + n * h * w].view(n, h, w))
        out = {"lm_loss": lm_loss}
        if gt_masks is not None:
            ce = dice = torch.zeros((), device=self.device)
            nm = 0
            for b in range(B):
                pm, gt = pred_masks[b], gt_masks[b].to(pred_masks[b])
                if pm.shape[-2:] != gt.shape[-2:]:
                    pm = F.interpolate(pm[None], size=gt.shape[-2:], mode="bilinear", align_corners=False)[0]
                ce = ce + sigmoid_ce_loss(pm, gt, gt.shape[0]) * gt.shape[0]
                dice = dice + dice_loss(pm, gt, gt.shape[0]) * gt.shape[0]
                nm += gt.shape[0]
            ce = self.bce_loss_weight * ce / (nm + 1e-8)
            dice = self.dice_loss_weight * dice / (nm + 1e-8)
            out.update({"loss": lm_loss + ce + dice, "ce_loss": ce, "dice_loss": dice, "mask_loss": ce + dice})
        if _return_extras:
            out.update(pred_masks=pred_masks, hidden=hid, logits=logits)
        return out


def _flat_ints(v):
    """ints of a scalar / list / tuple / tensor, flattened (a one-element list as `generate` takes it, or the bare value)"""
    return [int(x) for x in torch.as_tensor(v).reshape(-1).tolist()]


class _HostMergeStats(dict):
    """`model.adapter_stats` after a host-side `merge_adapter`: the merge's counts as a dict, as before adapter hot-swap; calling
    it gives the live handle's `adapter_stats()` like on any other model."""

    def __init__(self, counts, model):
        super().__init__(counts)
        self._model = model

    def __call__(self):
        return AnyRefForCausalLM.adapter_stats(self._model)


def _lora_bits():
    from .lora import TARGET_BITS
    return TARGET_BITS


class ImageSession:
    """`AnyRefForCausalLM.image_session(...)`: a context manager around `anyref_session_open` / `_generate` / `_close`."""

    def __init__(self, model: AnyRefForCausalLM, clip_image, sam_image, sam_resized_size, height, width, prefix_ids):
        from .session import check_prefix
        self.model = m = model
        self.prefix = check_prefix(prefix_ids.tolist() if hasattr(prefix_ids, "tolist") else prefix_ids)
        clip = clip_image.to(m.device, torch.float32).contiguous()
        sam = sam_image.to(m.device, torch.float32).contiguous()
        if clip.numel() != 3 * m.cfg.clip.image_size ** 2 or sam.numel() != 3 * m.cfg.sam.img_size ** 2:
            raise ValueError("an image session holds exactly one image: clip_image [3, S, S] and sam_image [3, S, S]")
        rs, hh, ww = _flat_ints(sam_resized_size), _flat_ints(height), _flat_ints(width)
        if len(rs) != 2 or len(hh) != 1 or len(ww) != 1:
            raise ValueError("an image session holds exactly one image: one (h, w) resized size, one height, one width")
        self.height, self.width = hh[0], ww[0]
        self.resized = (rs[0], rs[1])
        rs_t = torch.tensor(rs, dtype=torch.int32)
        os_t = torch.tensor([self.height, self.width], dtype=torch.int32)
        pre = torch.tensor(self.prefix, dtype=torch.long)
        m._check(m.lib.anyref_session_open(m.h, m._stream(), _ptr(clip), _ptr(sam), _ptr(pre), len(self.prefix), _ptr(rs_t),
                                           _ptr(os_t)), "session_open")
        self.open = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        if self.open and self.model.h:
            self.model._check(self.model.lib.anyref_session_close(self.model.h), "session_close")
        self.open = False

    def refine(self, query: int, seg: int, **kw):
        """`model.refine` for mask `seg` of query `query` of this session's last `generate`; the session stays open"""
        return self.model.refine(query, seg, **kw)

    @torch.no_grad()
    def generate(self, input_ids, audios=None, ref_images=None, max_new_tokens=128, attention_masks=None, draft_ids=None,
                 _return_extras: bool = False):
        """`model.generate` for Q <= max_batch queries about the session's image, same return shape; the Q-row answer is what Q
        plain calls on the full prompts return.  A row of `input_ids` is either a suffix (what follows the image placeholder) or
        a full prompt as the reference's data loader produces it, which must begin with the session's prefix and is cut there;
        a row that does not raises ValueError naming the row (anyref_amd/session.py).  `output_ids` are full rows: prefix +
        suffix + answer.  `audios` positions are looked up in the suffixes.  `draft_ids` as in `model.generate`;
        `set_draft_policy("last")` is NOT applied inside a session (consecutive queries about one image have different answers
        more often than consecutive images have).  `ref_images` is not served: its features come out of the CLIP tower
        (`encode_images`), a call that ends the session."""
        from .draft import normalize_drafts
        from .session import cut_rows
        m = self.model
        if not self.open:
            raise RuntimeError("session_generate: this image session was closed")
        if ref_images is not None:
            raise NotImplementedError("ref_images inside an image session: encode_images would end the session")
        ids, lens = m._rows(input_ids, attention_masks)
        suffixes = cut_rows([ids[b, : int(lens[b])].tolist() for b in range(ids.shape[0])], self.prefix)
        Q, Lmax = len(suffixes), max(len(r) for r in suffixes)
        if Q > m.max_batch:
            raise ValueError(f"batch {Q} > max_batch {m.max_batch} the handle was created for")
        suf = torch.zeros(Q, Lmax, dtype=torch.long)
        for b, r in enumerate(suffixes):
            suf[b, : len(r)] = torch.tensor(r, dtype=torch.long)
        slens = torch.tensor([len(r) for r in suffixes], dtype=torch.int32)
        extra, slots, n_extra = m._extra(suf, slens, audios, None)
        Lout = len(self.prefix) + Lmax + int(max_new_tokens)
        out_ids = torch.zeros(Q, Lout, dtype=torch.long)
        out_lens = torch.zeros(Q, dtype=torch.int32)
        out_nseg = torch.zeros(Q, dtype=torch.int32)
        offs = torch.zeros(Q, dtype=torch.long)
        height, width = [self.height] * Q, [self.width] * Q
        cap = Q * m.max_seg * self.height * self.width
        out_masks = torch.empty(cap, device=m.device, dtype=torch.float32)
        out_low = hid = None
        if _return_extras or m._sp_max:
            L = 4 * m.cfg.sam.grid
            out_low = torch.zeros(Q, m.max_seg, L, L, device=m.device, dtype=torch.float32)
            if _return_extras and _return_extras != "low":
                hid = torch.empty(Q, m.cfg.llm.max_seq, m.cfg.llm.dim, device=m.device, dtype=torch.float32)
        eos = m.config.eos_token_id if m.config.eos_token_id is not None else -1
        if draft_ids is not None:
            drafts = normalize_drafts(draft_ids, Q)
            if any(drafts):
                m.set_draft(drafts)
        pending = m._masks_begin([self.height] * Q, [self.width] * Q)
        m._check(m.lib.anyref_session_generate(
            m.h, m._stream(), _ptr(suf), _ptr(slens), Q, Lmax, _ptr(extra), _ptr(slots), n_extra, int(max_new_tokens), int(eos),
            _ptr(out_ids), _ptr(out_lens), _ptr(out_nseg), _ptr(out_masks), cap, _ptr(offs), _ptr(out_low), _ptr(hid)),
            "session_generate")
        m._generated(Q, max_new_tokens)
        m._masks_made(pending)
        m._refine_keep(out_low, [self.resized] * Q, height, width)
        res = m._result(out_ids, out_lens, out_nseg, offs, out_masks, height, width, per_row=True)
        if _return_extras:
            return res, dict(out_lens=out_lens, nseg=out_nseg, low_res=out_low, hidden=hid, **m.draft_stats(Q))
        return res


class PooledSession:
    """what `SessionPool.open` returns: one image resident in one slot of the pool.  `.slot`, `.key`, `.prefix` (the ids up to
    and including the image placeholder), `.height` / `.width`."""

    def __init__(self, pool, key, slot, gen, prefix, height, width):
        self.pool, self.key, self.slot, self.gen, self.prefix = pool, key, slot, gen, prefix
        self.height, self.width = height, width

    def check(self):
        """raises if the slot no longer holds this session (closed, evicted by a later `open`, or opened again)"""
        t = self.pool.table
        if t.slot_of(self.key) != self.slot or t.gens[self.slot] != self.gen:
            raise RuntimeError(f"pooled session {self.key!r} is gone from slot {self.slot}: it was closed, evicted as the least "
                               "recently used, its key was opened again, or a weight change (an adapter switch) ended the "
                               "pool's slots (pool.get(key) returns the current session or None)")


class SessionPool:
    """`AnyRefForCausalLM.session_pool(slots)`: many images resident at once, queries about different images in one call
    (`anyref_session_pool_reserve` / `_store` / `_generate_pooled`).  The host rules -- key to slot, least
    recently used eviction, generations, chunking, row placement -- are anyref_amd/session.py's."""

    def __init__(self, model: "AnyRefForCausalLM", slots: int, max_prefix_rows=None):
        from .session import SlotTable, default_max_prefix_rows
        self.model = m = model
        self.table = SlotTable(slots)
        self.max_prefix_rows = int(max_prefix_rows) if max_prefix_rows is not None else \
            default_max_prefix_rows(m.cfg.llm.max_seq, m.n_img)
        m._check(m.lib.anyref_session_pool_reserve(m.h, self.table.n_slots, self.max_prefix_rows), "session_pool_reserve")
        self._sessions = {}                       # key -> PooledSession
        self._held = [None] * m.max_batch         # (slot, generation) the cache rows held after the last pooled call
        self.closed = False

    def _live(self):
        if self.closed:
            raise RuntimeError("this session pool was closed (pool.close()): ask the model for a new one")

    def _forget_all(self):
        """every session is gone (the library ended the slots, or the pool was closed): keys released, generations bumped, so
        `get` returns None and a session object handed out before fails its `check`"""
        for key in self.table.lru_order():
            self.table.release(key)
        self._sessions.clear()
        self._held = [None] * self.model.max_batch

    def open(self, key, clip_image, sam_images, sam_resized_sizes, height, width, prefix_ids) -> PooledSession:
        """Encode the image (`model.image_session`'s open) and store it in a slot under `key`.  A key already held keeps its
        slot and is replaced; a full pool evicts the least recently used key, whose session object raises on its next use."""
        m = self.model
        self._live()
        sess = ImageSession(m, clip_image, sam_images, sam_resized_sizes, height, width, prefix_ids)
        P = len(sess.prefix) + m.n_img - 1
        if P > self.max_prefix_rows:
            sess.close()
            raise ValueError(f"the prefix splices to {P} rows, the pool was reserved for max_prefix_rows = {self.max_prefix_rows}")
        slot, evicted = self.table.assign(key)
        self._sessions.pop(evicted, None)
        try:
            m._check(m.lib.anyref_session_store(m.h, m._stream(), slot), "session_store")
        except Exception:
            self.table.release(key)               # (what the slot held before, if anything, goes with it: both sides agree)
            self._sessions.pop(key, None)
            m.lib.anyref_session_slot_close(m.h, slot)
            raise
        finally:
            sess.close()                          # the slot holds it now; the working buffers are free for any other call
        self._held = [None] * m.max_batch
        ps = PooledSession(self, key, slot, self.table.gens[slot], sess.prefix, sess.height, sess.width)
        ps.resized = sess.resized
        self._sessions[key] = ps
        return ps

    def get(self, key):
        """the session held under `key` (which becomes the most recently used), or None"""
        self._live()
        ps = self._sessions.get(key)
        if ps is not None:
            self.table.touch(key)
        return ps

    def close(self, key=None):
        """close the session held under `key`; without a key: every session, the pool's device memory is released and the
        pool refuses further use (`model.session_pool(...)` gives a new one)"""
        m = self.model
        if key is None:
            if self.closed:
                return
            self._forget_all()
            self.closed = True
            if m._session_pool is self:
                m._session_pool = None
            if m.h:
                m._check(m.lib.anyref_session_pool_reserve(m.h, 0, 0), "session_pool_reserve")
            return
        self._live()
        slot = self.table.release(key)
        self._sessions.pop(key, None)
        if slot is not None and m.h:
            m._check(m.lib.anyref_session_slot_close(m.h, slot), "session_slot_close")

    def stats(self) -> dict:
        """`anyref_session_pool_stats`: slots, in_use, bytes, rows the last pooled call gathered / skipped, its gather's
        device time in ms (None when it launched none)"""
        m = self.model
        i = [C.c_int32() for _ in range(4)]
        nb, ms = C.c_int64(), C.c_double()
        m._check(m.lib.anyref_session_pool_stats(m.h, C.byref(i[0]), C.byref(i[1]), C.byref(nb), C.byref(i[2]), C.byref(i[3]),
                                                 C.byref(ms)), "session_pool_stats")
        return dict(slots=i[0].value, in_use=i[1].value, bytes=nb.value, rows_gathered=i[2].value, rows_skipped=i[3].value,
                    gather_ms=None if ms.value < 0 else ms.value)

    @torch.no_grad()
    def generate(self, sessions, input_ids, audios=None, ref_images=None, max_new_tokens=128, attention_masks=None,
                 draft_ids=None, _return_extras: bool = False):
        """`ImageSession.generate` with one session per row: row b of `input_ids` is a question about `sessions[b]`, as a bare
        suffix or as a full prompt that begins with THAT session's prefix (a row that does not raises ValueError naming the
        row).  Rows may be about one image or about different images, at most max_batch of them.  Same return shape;
        `output_ids` rows are the row's own prefix + suffix + answer.  `ref_images` is not served, as in a session."""
        from .draft import normalize_drafts
        from .session import cut_rows_each
        m = self.model
        self._live()
        if ref_images is not None:
            raise NotImplementedError("ref_images inside a pooled session: encode_images needs the working buffers per call")
        sessions = list(sessions)
        for ps in sessions:
            ps.check()
        ids, lens = m._rows(input_ids, attention_masks)
        suffixes = cut_rows_each([ids[b, : int(lens[b])].tolist() for b in range(ids.shape[0])], [ps.prefix for ps in sessions])
        Q, Lmax = len(suffixes), max(len(r) for r in suffixes)
        if Q > m.max_batch:
            raise ValueError(f"batch {Q} > max_batch {m.max_batch} the handle was created for")
        suf = torch.zeros(Q, Lmax, dtype=torch.long)
        for b, r in enumerate(suffixes):
            suf[b, : len(r)] = torch.tensor(r, dtype=torch.long)
        slens = torch.tensor([len(r) for r in suffixes], dtype=torch.int32)
        slots = torch.tensor([ps.slot for ps in sessions], dtype=torch.int32)
        extra, eslots, n_extra = m._extra(suf, slens, audios, None)
        Lout = max(len(ps.prefix) for ps in sessions) + Lmax + int(max_new_tokens)
        out_ids = torch.zeros(Q, Lout, dtype=torch.long)
        out_lens = torch.zeros(Q, dtype=torch.int32)
        out_nseg = torch.zeros(Q, dtype=torch.int32)
        offs = torch.zeros(Q, dtype=torch.long)
        height, width = [ps.height for ps in sessions], [ps.width for ps in sessions]
        cap = sum(m.max_seg * h * w for h, w in zip(height, width))
        out_masks = torch.empty(cap, device=m.device, dtype=torch.float32)
        out_low = hid = None
        if _return_extras or m._sp_max:
            L = 4 * m.cfg.sam.grid
            out_low = torch.zeros(Q, m.max_seg, L, L, device=m.device, dtype=torch.float32)
            if _return_extras and _return_extras != "low":
                hid = torch.empty(Q, m.cfg.llm.max_seq, m.cfg.llm.dim, device=m.device, dtype=torch.float32)
        eos = m.config.eos_token_id if m.config.eos_token_id is not None else -1
        if draft_ids is not None:
            drafts = normalize_drafts(draft_ids, Q)
            if any(drafts):
                m.set_draft(drafts)
        pending = m._masks_begin(height, width)
        m._check(m.lib.anyref_session_generate_pooled(
            m.h, m._stream(), _ptr(slots), _ptr(suf), _ptr(slens), Q, Lmax, _ptr(extra), _ptr(eslots), n_extra,
            int(max_new_tokens), int(eos), _ptr(out_ids), _ptr(out_lens), _ptr(out_nseg), _ptr(out_masks), cap, _ptr(offs),
            _ptr(out_low), _ptr(hid)), "session_generate_pooled")
        m._generated(Q, max_new_tokens)
        m._masks_made(pending)
        m._refine_keep(out_low, [ps.resized for ps in sessions], height, width)
        for b, ps in enumerate(sessions):
            self.table.touch(ps.key)
            self._held[b] = (ps.slot, ps.gen)
        res = m._result(out_ids, out_lens, out_nseg, offs, out_masks, height, width, per_row=True)
        if _return_extras:
            return res, dict(out_lens=out_lens, nseg=out_nseg, low_res=out_low, hidden=hid, **m.draft_stats(Q))
        return res

    @torch.no_grad()
    def generate_many(self, items, max_new_tokens=128, _return_extras: bool = False):
        """Any number of `(session, ids)` items -- ids a 1-D suffix or full prompt -- answered in calls of at most max_batch rows.
        -> one `(output_ids [n], pred_masks [nseg, h, w] or None)` per item, in the caller's order (with `_return_extras`, a
        third entry: a dict with the row's `low_res`, `nseg` and, unless "low", `hidden`).  Items are taken in order, max_batch
        per call; inside a call an item is given the cache row that already holds its image from the call before where there is
        one (anyref_amd/session.py `plan_calls`), so that row's gather is skipped."""
        from .session import plan_calls
        self._live()
        items = [(ps, torch.as_tensor(ids).reshape(-1).long()) for ps, ids in items]
        for ps, _ in items:
            ps.check()
        out = [None] * len(items)
        scores = [None] * len(items) if self.model._scores_on else None
        reports = [None] * len(items) if self.model._reports_on else None
        for order in plan_calls([(ps.slot, ps.gen) for ps, _ in items], self.model.max_batch, self._held):
            rows = [items[i][1] for i in order]
            n = max(len(r) for r in rows)
            ids = torch.zeros(len(rows), n, dtype=torch.long)
            mask = torch.zeros(len(rows), n, dtype=torch.bool)
            for b, r in enumerate(rows):
                ids[b, : len(r)] = r
                mask[b, : len(r)] = True
            res, ex = self.generate([items[i][0] for i in order], ids, attention_masks=mask, max_new_tokens=max_new_tokens,
                                    _return_extras=_return_extras or "low")
            if scores is not None:                # (the next call clears them)
                for b, e in enumerate(self.model._read_token_scores()):
                    scores[order[b]] = e
            if reports is not None:
                for b, e in enumerate(self.model._read_mask_reports()):
                    reports[order[b]] = e
            for b, i in enumerate(order):
                n_ids, nseg = int(ex["out_lens"][b]), int(ex["nseg"][b])
                one = (res[0][b, :n_ids], res[1][b] if res[1] is not None and nseg > 0 else None)
                if _return_extras:
                    one += (dict(low_res=ex["low_res"][b], nseg=nseg, hidden=None if ex["hidden"] is None else ex["hidden"][b]),)
                out[i] = one
        self.model._scores_many = scores
        self.model._reports_many = reports
        return out


def dice_loss(inputs, targets, num_masks, scale=1000, eps=1e-6):
    """`dice_loss` (model/anyref.py:19-47): the live body adds 1 to numerator and denominator and divides by
    `num_masks`; `scale` / `eps` are dead arguments there (the scaled variant is commented out, :38-42)."""
    inputs = inputs.sigmoid().flatten(1, 2)
    targets = targets.flatten(1, 2)
    numerator = 2 * (inputs * targets).sum(-1)
    denominator = inputs.sum(-1) + targets.sum(-1)
    loss = 1 - (numerator + 1) / (denominator + 1)
    return loss.sum() / num_masks


def sigmoid_ce_loss(inputs, targets, num_masks):
    """`sigmoid_ce_loss` (model/anyref.py:51-68)."""
    loss = F.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    return loss.flatten(1, 2).mean(1).sum() / (num_masks + 1e-8)
