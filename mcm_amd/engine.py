"""NativeCLIP — the `net` object of the reference's hot path, backed by libmcm_hip.so.

Mirrors the duck-typed model contract the reference relies on
(utils/detection_util.py:225,229-230; eval_ood_detection.py:61):

    net.eval()
    net.get_image_features(pixel_values=FloatTensor[b,3,S,S] on device) -> Tensor[b,P]
    net.get_text_features(input_ids=LongTensor[K,S], attention_mask=LongTensor[K,S]) -> Tensor[K,P]

returning real, writable fp32 tensors (the reference calls `.float()` and in-place `/=`
on them), plus the fused path `score_images` that the re-written `get_ood_scores_clip`
uses so the [B,K] softmax never leaves the GPU.

PyTorch is plumbing only: it owns device buffers and the current HIP stream; every FLOP
of the path runs in the hand-written gfx950 kernels behind the C ABI (include/mcm.h).
There is no CPU or eager fallback — a missing library or GPU raises.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Dict, Optional

import numpy as np

from . import abi
from .config import (ABI_VERSION, ClipGeometry, DT_BF16, DT_F16, DT_F32, PREC_BF16, PREC_F16, PREC_F32, SCORE_KINDS,
                     WEIGHT_OPERANDS, geometry)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmcm_hip.so")
# the same sources built with -DMCM_HARNESS: A/B kernel arms + mcm_debug_* switches; tests and tools only
HARNESS_LIB_PATH = os.path.join(_HERE, "libmcm_hip_harness.so")
# what libmcm_hip.so exports, and what only the harness library does: the declarations of include/mcm.h
EXPORTED_SYMBOLS = list(abi.PROTOTYPES)
HARNESS_ONLY_SYMBOLS = list(abi.HARNESS_PROTOTYPES)
# MCM_KC_* in the order of mcm_profile_read's arrays, lower-cased; gemm_*: sub-classes of "gemm" (MCM_KC_GEMM_*)
KERNEL_CLASSES = [name[len("MCM_KC_"):].lower() for name in sorted(abi.DEFINES, key=abi.DEFINES.get)
                  if name.startswith("MCM_KC_") and name != "MCM_KC_COUNT"]
TOPK_MAX = abi.DEFINES["MCM_TOPK_MAX"]  # concepts the top-k scoring tail returns per image
MAX_SPLITS = abi.DEFINES["MCM_KNN_MAX_SPLITS"]  # ranges a bank-streamed score cuts its bank into, at most

_libs = {}


class NativeLibraryMissing(RuntimeError):
    pass


def load_library(harness: bool = False):
    """dlopen libmcm_hip.so and declare the C ABI (include/mcm.h).  Raises loudly when the
    extension has not been built — the product path has no fallback.  `harness=True` loads
    libmcm_hip_harness.so instead (A/B tests and tools: extra kernel arms and the mcm_debug_* switches)."""
    if harness in _libs:
        return _libs[harness]
    path = HARNESS_LIB_PATH if harness else LIB_PATH
    if not os.path.exists(path):
        raise NativeLibraryMissing(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C mcm_amd/csrc).  mcm_amd has no CPU fallback.")
    # Both this library and PyTorch link libamdhip64, each from its own ROCm tree.  Whichever is loaded first provides the
    # HIP runtime of the process; when ours (/opt/rocm) came first, torch's later calls failed with "no ROCm-capable device
    # is detected" (measured).  The host code that owns buffers and streams here is torch's, so torch goes first when it
    # is installed; a torch-less process (tests/c_abi) simply runs on /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = abi.declare(ctypes.CDLL(path), harness=harness)
    if L.mcm_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version {L.mcm_abi_version()}, this package speaks {ABI_VERSION} — rebuild (make -C mcm_amd/csrc)")
    _libs[harness] = L
    return L


def _stream_ptr():
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pixel_format(px) -> int:
    """MCM_PIXELS_* of pixels as `NativeCLIP._pixels` returns them."""
    import torch

    return abi.DEFINES["MCM_PIXELS_U8_NHWC" if px.dtype == torch.uint8 else "MCM_PIXELS_F32_NCHW"]


def _int32_ids(a):
    """[K,S] token ids or slots, tensor or array, as a contiguous int32 host array."""
    return np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a), dtype=np.int32)


def _at(t, s, n):
    """The pointer of rows [s, s + n) of an optional output tensor: None where there is none."""
    return None if t is None else t[s:s + n].data_ptr()


class NativeCLIP:
    """CLIP towers + MCM scoring tail on one MI355X."""

    def __init__(self, geo: ClipGeometry | str, state_dict: Dict[str, np.ndarray], *,
                 device: int = 0, precision: str = "fp16", max_batch: int = 512,
                 max_prompt_tokens: int = 1024 * 77, synthetic_weights: Optional[bool] = None,
                 harness: bool = False, weight_operands: str = "auto", x2_max_batch: Optional[int] = None):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("NativeCLIP needs a HIP device (no CPU fallback)")
        self.geo = geometry(geo) if isinstance(geo, str) else geo
        self.device = torch.device("cuda", device)
        # "fp16x2": an fp16 handle whose `score_images` / `get_image_features` run the split-activation arm (mcm_score_x2) —
        # every score at fp32-grade accuracy (within one fp32 ulp of the fp32 arm) at about half the fp16 arm's throughput
        self.x2_default = precision == "fp16x2"
        self.precision = {"bf16": PREC_BF16, "fp32": PREC_F32, "f32": PREC_F32, "fp16": PREC_F16,
                          "f16": PREC_F16, "fp16x2": PREC_F16}[precision]
        self.max_batch = int(max_batch)
        # True: seeded stand-in parameters (the hash tokenizer stand-in is then acceptable); False: a real
        # checkpoint (it is refused); None: the caller did not say (mcm_amd.detection falls back to args.weights)
        self.synthetic_weights = synthetic_weights
        self._lib = load_library(harness)  # harness=True: A/B tests and tools only
        torch.cuda.set_device(self.device)
        torch.cuda.init()
        # 16-bit modes: how a GEMM weight is held (include/mcm.h MCM_WEIGHTS_*).  "auto": one 16-bit operand when every
        # weight IS a number of that dtype (the reference's fp16-trained checkpoints), W_hi + W_lo otherwise
        self._cfg = self.geo.to_c(device=device, precision=self.precision, max_batch=max_batch,
                                  max_prompt_tokens=max_prompt_tokens,
                                  weight_operands=WEIGHT_OPERANDS[weight_operands],
                                  # the split-activation workspace (fp16 handles; include/mcm.h mcm_config.x2_max_batch): None /
                                  # 0 = the arm runs at the full batch (twice the activation bytes), n = at most n images per
                                  # x2 call (free up to max_batch / 2), < 0 = none
                                  x2_max_batch=int(x2_max_batch or 0))
        self._h = ctypes.c_void_p()
        rc = self._lib.mcm_create(ctypes.byref(self._cfg), ctypes.byref(self._h))
        if rc:
            raise RuntimeError(f"mcm_create rc={rc}: {self._lib.mcm_last_error(None).decode()}")
        for name, arr in state_dict.items():
            if name == "logit_scale" or name.endswith("position_ids"):
                continue  # unused by MCM (reference utils/detection_util.py:232) / HF buffers
            arr = np.asarray(arr)
            if arr.dtype == np.float16:  # an fp16 checkpoint is handed over as it is (the library widens exactly)
                a, dt = np.ascontiguousarray(arr), DT_F16
            elif str(arr.dtype) == "bfloat16":  # ml_dtypes / safetensors views: raw 16-bit patterns
                a, dt = np.ascontiguousarray(arr).view(np.uint16), DT_BF16
            else:
                a, dt = np.ascontiguousarray(arr, dtype=np.float32), DT_F32
            shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
            self._check(self._lib.mcm_set_weight(self._h, name.encode(), a.ctypes.data_as(ctypes.c_void_p), dt,
                                                 shape, a.ndim))
        self._check(self._lib.mcm_finalize_weights(self._h))
        n, sp = ctypes.c_uint64(0), ctypes.c_int32(0)
        self._check(self._lib.mcm_weights_operand_exact(self._h, ctypes.byref(n), ctypes.byref(sp)))
        # vision GEMM-weight elements that are not numbers of the operand dtype, and whether the split-weight
        # GEMMs run (weight_operands="auto": exactly when that count is non-zero)
        self.weights_inexact, self.split_weights = int(n.value), bool(sp.value)

    # -- plumbing ------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc:
            raise RuntimeError(f"libmcm_hip rc={rc}: {self._lib.mcm_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mcm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def eval(self):  # reference eval_ood_detection.py:61
        return self

    def _pixels(self, pixel_values):
        import torch

        S = self.geo.image_size
        if pixel_values.dtype == torch.uint8:  # NHWC uint8 ingest (fused /255 + normalise)
            if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (S, S, 3):
                raise ValueError(f"uint8 input must be [b,{S},{S},3] NHWC, got {tuple(pixel_values.shape)}")
            return pixel_values.to(device=self.device).contiguous()
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, S, S):
            # HF modeling_clip.py:204-207 raises ValueError on a wrong image size
            raise ValueError(f"Input image size {tuple(pixel_values.shape)} doesn't match model (3x{S}x{S}).")
        return pixel_values.to(device=self.device, dtype=torch.float32).contiguous()

    @staticmethod
    def _chunks(b, nb):
        """(start, n) of the chunks of at most nb that b images go through a fixed workspace in."""
        for s in range(0, b, nb):
            yield s, min(nb, b - s)

    def _in_chunks(self, b, nb, call):
        """call(start, n) -> rc over the chunks of at most nb that b images go through a fixed workspace in."""
        for s, n in self._chunks(b, nb):
            self._check(call(s, n))

    def _empty(self, *shape, dtype=None, when=True):
        """An uninitialised device tensor (fp32 unless `dtype`), or None for an output nobody asked for (`when` false)."""
        import torch

        return torch.empty(shape, device=self.device, dtype=dtype or torch.float32) if when else None

    def _x2_batch(self):
        """`x2_max_batch` where the split-activation arm exists."""
        nb = self.x2_max_batch
        if nb <= 0:
            raise RuntimeError("the split-activation arm needs an fp16 handle")
        return nb

    # -- the model contract ----------------------------------------------------------------
    def get_image_features(self, pixel_values, normalize: bool = False):
        """[b,3,S,S] fp32 (or [b,S,S,3] uint8) → [b,P] fp32.  With the default `normalize=False` this is
        exactly what HF `CLIPModel.get_image_features` returns — the projection output, NOT unit-norm —
        so unmodified reference code that normalises (or, for the Mahalanobis baseline, deliberately
        does not normalise) the rows itself gets what it expects (utils/detection_util.py:158,187,225).
        `normalize=True` fuses the reference's `/= norm` (:226) into the pooling kernel."""
        if self.x2_default:
            return self.get_image_features_x2(pixel_values, normalize=normalize)
        px = self._pixels(pixel_values)
        return self._encode_into(px, self._empty(px.shape[0], self.geo.proj_dim), normalize, x2=False)

    def _encode_into(self, px, out, normalize: bool, x2: bool):
        """The image tower over `px` (as `_pixels` returns them) into out [b,P], in chunks of the arm's largest batch."""
        fmt = _pixel_format(px)
        fn = self._lib.mcm_encode_image_x2 if x2 else self._lib.mcm_encode_image_ex
        self._in_chunks(px.shape[0], self._x2_batch() if x2 else self.max_batch, lambda s, n: fn(
            self._h, px[s:s + n].data_ptr(), fmt, n, int(bool(normalize)), out[s:s + n].data_ptr(), _stream_ptr()))
        return out

    def get_image_features_raw(self, pixel_values):
        """Alias of `get_image_features(pixel_values)` (kept for round-1 callers)."""
        return self.get_image_features(pixel_values, normalize=False)

    def maha_prepare(self, classwise_mean, precision):
        """(means [C,P], precision [P,P]) → opaque state for `maha_scores`."""
        import torch

        mu = classwise_mean.to(device=self.device, dtype=torch.float32).contiguous()
        pr = precision.to(device=self.device, dtype=torch.float32).contiguous()
        C, P = mu.shape
        assert P == self.geo.proj_dim and pr.shape == (P, P)
        w = torch.empty((C, P), device=self.device, dtype=torch.float64)
        k = torch.empty((C,), device=self.device, dtype=torch.float64)
        self._check(self._lib.mcm_maha_prepare(self._h, mu.data_ptr(), pr.data_ptr(), C, w.data_ptr(),
                                               k.data_ptr(), _stream_ptr()))
        return {"prec": pr, "w": w, "k": k, "C": C}

    def maha_scores(self, features, state):
        """features [B,P] fp32 (device) → [B] fp32: min_c 0.5 (f-mu_c) P (f-mu_c)^T."""
        import torch

        f = features.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty(f.shape[0], device=self.device, dtype=torch.float32)
        self._check(self._lib.mcm_maha_score_features(self._h, f.data_ptr(), f.shape[0], state["prec"].data_ptr(),
                                                      state["w"].data_ptr(), state["k"].data_ptr(), state["C"],
                                                      out.data_ptr(), _stream_ptr()))
        return out

    def maha_fit_state(self, shift=None):
        """Zeroed running statistics of the Mahalanobis fit: {gram [P,P] fp64, sum [P] fp64, shift [P] fp32, n}, device
        tensors; `shift` (default 0) is subtracted from every feature row before it is accumulated (include/mcm.h
        mcm_maha_fit_accumulate: it is there for the error, the covariance does not depend on it)."""
        import torch

        P = self.geo.proj_dim
        sh = (torch.zeros(P, device=self.device, dtype=torch.float32) if shift is None
              else shift.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous())
        if sh.shape != (P,):
            raise ValueError(f"shift must hold proj_dim = {P} values, got {tuple(sh.shape)}")
        return {"gram": torch.zeros((P, P), device=self.device, dtype=torch.float64),
                "sum": torch.zeros(P, device=self.device, dtype=torch.float64), "shift": sh, "n": 0}

    def maha_fit_accumulate(self, features, state):
        """features [B,P] fp32 → state: gram += sum_b x x^T, sum += sum_b x with x = f_b - shift, n += B.  One launch."""
        import torch

        f = features.to(device=self.device, dtype=torch.float32).contiguous()
        if f.dim() != 2 or f.shape[1] != self.geo.proj_dim:
            raise ValueError(f"features must be [B, {self.geo.proj_dim}], got {tuple(f.shape)}")
        self._check(self._lib.mcm_maha_fit_accumulate(self._h, f.data_ptr(), f.shape[0], state["shift"].data_ptr(),
                                                      state["gram"].data_ptr(), state["sum"].data_ptr(), _stream_ptr()))
        state["n"] += int(f.shape[0])
        return state

    def knn_scores(self, features, bank, k, splits: int = 0, return_values: bool = False):
        """features [B,P], bank [N,P] fp32 (device) → [B] fp32: sqrt(max(0, 2 - 2 v_k)), v_k the k-th largest fp32 dot
        product of the row with the bank's rows — for unit-norm rows the distance to the k-th nearest neighbour (include/mcm.h
        mcm_knn_score_features).  `splits`: 0 = the library's choice, n = the bank in exactly n ranges (a tuning argument: the
        result does not depend on it).  `return_values=True`: (scores, topv [B,k]), the k largest similarities, descending,
        -inf where the bank has no candidate left.  The workspace is a buffer of this object that grows on demand; queries
        go through in blocks of at most 4096 rows."""
        f, bk = self._bank_operands(features, bank)
        k, splits = int(k), int(splits)
        B, N, max_k = int(f.shape[0]), int(bk.shape[0]), abi.DEFINES["MCM_KNN_MAX_K"]
        scores, topv = self._empty(B), self._empty(B, max(k, 0), when=return_values)
        self._bank_score(
            "knn_scores", "_knn_work", B,
            lambda n: self._rules(B=n, N=N, splits=splits) + [(f"k={k} (1 <= k <= {max_k})", not 1 <= k <= max_k)],
            lambda n, need: self._lib.mcm_knn_workspace_bytes(self._h, n, N, k, splits, need),
            lambda s, n, work: self._lib.mcm_knn_score_features(
                self._h, f[s:s + n].data_ptr(), n, bk.data_ptr(), N, k, splits, work.data_ptr(), work.numel() * 4,
                scores[s:s + n].data_ptr(), _at(topv, s, n), _stream_ptr()))
        return (scores, topv) if return_values else scores

    def _bank_operands(self, features, bank):
        """(features, bank) as contiguous fp32 device tensors, both [*, proj_dim] (the operands of a bank-streamed score)."""
        import torch

        f = features.to(device=self.device, dtype=torch.float32).contiguous()
        bk = bank.to(device=self.device, dtype=torch.float32).contiguous()
        P = self.geo.proj_dim
        if f.dim() != 2 or f.shape[1] != P or bk.dim() != 2 or bk.shape[1] != P:
            raise ValueError(f"features and bank must be [*, {P}], got {tuple(f.shape)} and {tuple(bk.shape)}")
        return f, bk

    def _bank_score(self, what, slot, B, rules, ask, launch):
        """The B queries of a bank-streamed score in blocks of at most 4096 rows: ask(n, byref(int64)) -> rc asks the library
        what a block of n needs, launch(start, n, work) -> rc scores the block on the workspace of `slot`; rules(n) are the
        score's rules for a block of n, by which `_refusal` explains a refused call."""
        for s in range(0, max(B, 1), 4096):
            n = min(4096, B - s)
            work = self._workspace(slot, lambda need: self._refusal(what, ask(n, need), rules(n)))
            self._refusal(what, launch(s, n, work), rules(n))

    def _workspace(self, slot, ask):
        """The workspace of a score: the buffer kept in the attribute `slot`, replaced by a larger one where it holds less
        than ask(byref(int64)) says the call needs.  One buffer per score, since two scores may be in flight on two streams."""
        need = ctypes.c_int64(0)
        ask(ctypes.byref(need))
        work = getattr(self, slot, None)
        if work is None or work.numel() * 4 < need.value:
            work = self._empty((need.value + 3) // 4)
            setattr(self, slot, work)
        return work

    def _rules(self, T=None, splits=None, **at_least_1):
        """The rules the bank-streamed scores share, as `_refusal` reads them: every keyword at least 1, T positive and
        finite, splits within the header's range (either where given), and the walk's proj_dim % 4 == 0."""
        P = self.geo.proj_dim
        rules = [(f"{name}={v} ({name} >= 1)", v < 1) for name, v in at_least_1.items()]
        if T is not None:
            rules.append((f"T={T} (positive and finite)", not (T > 0 and math.isfinite(T))))
        if splits is not None:
            rules.append((f"splits={splits} (0 <= splits <= {MAX_SPLITS})", not 0 <= splits <= MAX_SPLITS))
        return rules + [(f"proj_dim={P} (proj_dim % 4 == 0)", P % 4 != 0)]

    def _refusal(self, what, rc, rules):
        """The one path of a bank-streamed score's return code.  MCM_EINVAL is a refusal of the arguments: ValueError naming
        the violated ones of `rules`, (text, violated) pairs with text = "name=value (the rule)"; where none is, every value
        and the library's own message.  Any other failure is not about the arguments: RuntimeError through `_check`."""
        if rc != abi.DEFINES["MCM_EINVAL"]:
            return self._check(rc)
        bad = [text for text, violated in rules if violated]
        raise ValueError(f"{what}: refused (rc={rc}): " + ("; ".join(bad) if bad else
                         ", ".join(text.split(" (")[0] for text, _ in rules) + ": " + self._lib.mcm_last_error(self._h).decode()))

    def neglabel_scores(self, features, bank, n_id, groups, group_size, T: float = 0.01, splits: int = 0,
                        return_groups: bool = False):
        """features [B,P], bank [n_id + groups * group_size, P] fp32 (device) → [B] fp32: the NegLabel score -(1/G) sum_g S_g,
        S_g = 1 / (1 + exp(LN_g - LI)) the softmax mass at temperature T of the bank's first n_id rows (the ID prompts) against
        negative group g alone (include/mcm.h mcm_neglabel_score_features); larger = more OOD.  `splits`: 0 = the library's
        choice, n = the bank in exactly n ranges (results agree across it to rounding, and are the same bits for a fixed
        value).  `return_groups=True`: (scores, S [B,groups]).  The workspace is a buffer of this object that grows on
        demand; queries go through in blocks of at most 4096 rows."""
        f, bk = self._bank_operands(features, bank)
        K, G, gs, splits, T = int(n_id), int(groups), int(group_size), int(splits), float(T)
        if K < 1 or G < 1 or gs < 1 or bk.shape[0] != K + G * gs:
            raise ValueError(f"neglabel_scores: the bank has {bk.shape[0]} rows, n_id + groups * group_size = {K} + {G} * {gs}")
        B, max_g = int(f.shape[0]), abi.DEFINES["MCM_NEG_MAX_GROUPS"]
        scores, grp = self._empty(B), self._empty(B, G, when=return_groups)
        self._bank_score(
            "neglabel_scores", "_neg_work", B,
            lambda n: self._rules(B=n, n_id=K, group_size=gs, T=T, splits=splits) + [
                (f"groups={G} (1 <= groups <= {max_g})", not 1 <= G <= max_g),
                (f"n_id + groups * group_size = {K + G * gs} (at most 2^31 - 1)", K + G * gs > 2 ** 31 - 1)],
            lambda n, need: self._lib.mcm_neglabel_workspace_bytes(self._h, n, K, G, gs, splits, need),
            lambda s, n, work: self._lib.mcm_neglabel_score_features(
                self._h, f[s:s + n].data_ptr(), n, bk.data_ptr(), K, G, gs, T, splits, work.data_ptr(), work.numel() * 4,
                scores[s:s + n].data_ptr(), _at(grp, s, n), _stream_ptr()))
        return (scores, grp) if return_groups else scores

    def vim_scores(self, features, bank, n_id, T: float = 0.01, alpha: float = 1.0, off=None, splits: int = 0,
                   return_parts: bool = False):
        """features [B,P], bank [n_id + R, P] fp32 (device) → [B] fp32: the ViM score alpha * resid - lse, resid the norm of the
        row's projections on the bank's last R rows (the null-space basis; minus `off` [R] fp64 where given), lse the
        log-sum-exp at temperature T of its dot products with the first n_id rows (the prompts) (include/mcm.h
        mcm_vim_score_features); larger = more OOD.  `splits`: 0 = the library's choice, n = the bank in exactly n ranges
        (results agree across it to rounding, and are the same bits for a fixed value).  `return_parts=True`: (scores,
        parts [B,3] = resid, lse, maxlogit).  The workspace is a buffer of this object that grows on demand; queries go through
        in blocks of at most 4096 rows."""
        import torch

        f, bk = self._bank_operands(features, bank)
        K, splits, T, alpha = int(n_id), int(splits), float(T), float(alpha)
        R = int(bk.shape[0]) - K
        if K < 1 or R < 1:
            raise ValueError(f"vim_scores: the bank has {bk.shape[0]} rows, n_id = {K}: both n_id and the basis rows behind "
                             "them must be at least 1")
        o = None
        if off is not None:
            o = off.to(device=self.device, dtype=torch.float64).reshape(-1).contiguous()
            if o.shape != (R,):
                raise ValueError(f"vim_scores: off must hold R = {R} values, got {tuple(o.shape)}")
        B = int(f.shape[0])
        scores, parts = self._empty(B), self._empty(B, 3, when=return_parts)
        self._bank_score(
            "vim_scores", "_vim_work", B,
            lambda n: self._rules(B=n, n_id=K, R=R, T=T, splits=splits) + [
                (f"n_id + R = {K + R} (at most 2^31 - 1)", K + R > 2 ** 31 - 1),
                (f"alpha={alpha} (finite)", not math.isfinite(alpha))],
            lambda n, need: self._lib.mcm_vim_workspace_bytes(self._h, n, K, R, splits, need),
            lambda s, n, work: self._lib.mcm_vim_score_features(
                self._h, f[s:s + n].data_ptr(), n, bk.data_ptr(), K, R, _at(o, 0, R), T, alpha, splits, work.data_ptr(),
                work.numel() * 4, scores[s:s + n].data_ptr(), _at(parts, s, n), _stream_ptr()))
        return (scores, parts) if return_parts else scores

    # -- GL-MCM: the local (patch-level) term next to MCM (include/mcm.h mcm_score_glmcm) -------------------
    @property
    def local_rows(self) -> int:
        """R: patch tokens per image, the rows of an image's local features."""
        return (self.geo.image_size // self.geo.patch_size) ** 2

    def _no_x2_local(self, what):
        if self.x2_default:
            raise ValueError(f"{what}: the split-activation arm (precision='fp16x2') has no local pass")

    def get_local_features(self, pixel_values):
        """[b,3,S,S] fp32 (or [b,S,S,3] uint8) → (global [b,P], local [b,R,P]) fp32, unit-norm rows: the global feature of
        `get_image_features(..., normalize=True)` (the same bits) and, per patch token, the last layer's value path
        (layer_norm1 → v_proj → out_proj → post_layernorm → visual_projection; include/mcm.h mcm_encode_image_local)."""
        self._no_x2_local("get_local_features")
        px = self._pixels(pixel_values)
        fmt = _pixel_format(px)
        b, R, P = px.shape[0], self.local_rows, self.geo.proj_dim
        glob, loc = self._empty(b, P), self._empty(b, R, P)
        self._in_chunks(b, self.max_batch, lambda s, n: self._lib.mcm_encode_image_local(
            self._h, px[s:s + n].data_ptr(), fmt, n, glob[s:s + n].data_ptr(), loc[s:s + n].data_ptr(), _stream_ptr()))
        return glob, loc

    def local_scores(self, local, text_features, T: float = 1.0, return_patches: bool = False):
        """local [B,R,P] + bank [K,P] fp32 (device) → [B] fp32: -S_L, S_L = max over the R rows of max_k softmax_k(row · bank / T)
        (include/mcm.h mcm_local_score_features); larger = more OOD.  `return_patches=True`: (scores, patch [B,R]), every
        row's largest softmax probability."""
        import torch

        loc = local.to(device=self.device, dtype=torch.float32).contiguous()
        t = self._bank(text_features)
        if loc.dim() != 3 or loc.shape[2] != self.geo.proj_dim or loc.shape[0] == 0 or loc.shape[1] == 0:
            raise ValueError(f"local must be [B,R,{self.geo.proj_dim}] with B, R >= 1, got {tuple(loc.shape)}")
        B, R, K, T = int(loc.shape[0]), int(loc.shape[1]), int(t.shape[0]), float(T)
        rules = self._rules(B=B, R=R, K=K, T=T) + [(f"B R = {B * R} (below 2^31)", B * R > 2 ** 31 - 1)]
        work = self._workspace("_local_work", lambda need: self._refusal(
            "local_scores", self._lib.mcm_local_workspace_bytes(self._h, B, R, K, need), rules))
        scores, patch = self._empty(B), self._empty(B, R, when=return_patches)
        self._refusal("local_scores", self._lib.mcm_local_score_features(
            self._h, loc.data_ptr(), B, R, t.data_ptr(), K, T, work.data_ptr(), work.numel() * 4, scores.data_ptr(),
            _at(patch, 0, B), _stream_ptr()), rules)
        return (scores, patch) if return_patches else scores

    def score_images_glmcm(self, pixel_values, text_features, T: float = 1.0, lam: float = 1.0, return_parts: bool = False):
        """pixels + pre-encoded bank [K,P] → the GL-MCM score [b] fp32 on the device: -(S_G + lam S_L), S_G the MCM term of
        the global feature (the bits of `score_images(..., "MCM")`), S_L the local term of `local_scores` on this image's
        patch rows (include/mcm.h mcm_score_glmcm); larger = more OOD.  `return_parts=True`: (scores, -S_G [b], -S_L [b],
        patch [b,R])."""
        self._no_x2_local("score_images_glmcm")
        px = self._pixels(pixel_values)
        fmt = _pixel_format(px)
        t = self._bank(text_features)
        b, R = px.shape[0], self.local_rows
        out = self._empty(b)
        gs, ls, patch = (self._empty(*shape, when=return_parts) for shape in ((b,), (b,), (b, R)))
        self._in_chunks(b, self.max_batch, lambda s, n: self._lib.mcm_score_glmcm(
            self._h, px[s:s + n].data_ptr(), fmt, n, t.data_ptr(), t.shape[0], float(T), float(lam), out[s:s + n].data_ptr(),
            _at(gs, s, n), _at(ls, s, n), _at(patch, s, n), _stream_ptr()))
        return (out, gs, ls, patch) if return_parts else out

    def get_text_features(self, input_ids, attention_mask=None, normalize: bool = False):
        """[K,S] ids → [K,P] fp32: HF `get_text_features` (the text projection output; unit-norm rows
        only with `normalize=True`, which fuses utils/detection_util.py:231).  `attention_mask` is
        accepted for signature parity and ignored: the mask is causal and the pooled row is the first
        EOS, so pads never influence it (golden KAT)."""
        import torch

        ids = _int32_ids(input_ids)
        if ids.ndim != 2:
            raise ValueError("input_ids must be [K,S]")
        K, S = ids.shape
        if S > self.geo.max_positions:  # HF modeling_clip.py:241-245
            raise ValueError(f"Sequence length must be less than max_position_embeddings (got {S})")
        out = torch.empty((K, self.geo.proj_dim), device=self.device, dtype=torch.float32)
        self._check(self._lib.mcm_encode_text_ex(self._h, ids.ctypes.data_as(ctypes.c_void_p), K, S,
                                                 int(bool(normalize)), out.data_ptr(), _stream_ptr()))
        return out

    def get_text_features_ctx(self, input_ids, slots, ctx, normalize: bool = False):
        """`get_text_features` with learned context vectors in place of some token embeddings (CoOp's `PromptLearner.forward` +
        `TextEncoder.forward`; include/mcm.h mcm_encode_text_ctx).  input_ids, slots: [K,S]; slots[k,s] = -1 for an ordinary
        token, j in [0, n_ctx) for row j of the prompt's context, the id under it being a placeholder that only pooling reads.
        ctx: tensor or array of any float dtype, [n_ctx, t_width] (one context for every prompt) or [K, n_ctx, t_width] (one
        per prompt); it is widened exactly to fp32.  Returns [K,P] fp32, unit-norm rows with `normalize=True`."""
        import torch

        ids = _int32_ids(input_ids)
        slot = _int32_ids(slots)
        if ids.ndim != 2 or slot.shape != ids.shape:
            raise ValueError("input_ids and slots must both be [K,S]")
        K, S = ids.shape
        if S > self.geo.max_positions:  # HF modeling_clip.py:241-245
            raise ValueError(f"Sequence length must be less than max_position_embeddings (got {S})")
        c = ctx if hasattr(ctx, "detach") else torch.from_numpy(np.ascontiguousarray(ctx))
        if not c.is_floating_point():
            raise ValueError(f"ctx must be a float tensor or array, got {c.dtype}")
        if c.dim() not in (2, 3) or c.shape[-1] != self.geo.t_width or c.shape[-2] < 1:
            raise ValueError(f"ctx must be [n_ctx,{self.geo.t_width}] or [K,n_ctx,{self.geo.t_width}], got {tuple(c.shape)}")
        if c.dim() == 3 and c.shape[0] != K:
            raise ValueError(f"a per-prompt ctx needs one context per prompt: first dimension {c.shape[0]}, K = {K}")
        c = c.detach().to(device=self.device, dtype=torch.float32).contiguous()  # (every 16-bit float is an fp32 number)
        out = torch.empty((K, self.geo.proj_dim), device=self.device, dtype=torch.float32)
        self._check(self._lib.mcm_encode_text_ctx(self._h, ids.ctypes.data_as(ctypes.c_void_p),
                                                  slot.ctypes.data_as(ctypes.c_void_p), K, S, c.data_ptr(), int(c.shape[-2]),
                                                  K if c.dim() == 3 else 1, int(bool(normalize)), out.data_ptr(), _stream_ptr()))
        return out

    # -- fused hot-loop body -----------------------------------------------------------------
    def _bank(self, text_features):
        """The prompt bank as the kernels read it: fp32, contiguous, on this device, [K, proj_dim],
        unit-norm rows are the caller's responsibility (get_text_features(normalize=True))."""
        import torch

        t = text_features.to(device=self.device, dtype=torch.float32).contiguous()
        if t.dim() != 2 or t.shape[1] != self.geo.proj_dim or t.shape[0] == 0:
            raise ValueError(f"text_features must be [K,{self.geo.proj_dim}], got {tuple(t.shape)}")
        return t

    def _topk_out(self, b: int, topk: int):
        """(scores [b] fp32, idx [b,topk] int32, prob [b,topk] fp32) on the device for the top-k tail."""
        import torch

        if not 1 <= int(topk) <= TOPK_MAX:
            raise ValueError(f"topk must be 1..{TOPK_MAX} (0: scores only), got {topk}")
        return self._empty(b), self._empty(b, int(topk), dtype=torch.int32), self._empty(b, int(topk))

    def _score_images_topk(self, pixel_values, text_features, T, score, topk, x2: bool):
        """`score_images` / `score_images_x2` with the top-k tail (mcm_score_topk), in chunks of the arm's largest batch."""
        nb = self._x2_batch() if x2 else self.max_batch
        px = self._pixels(pixel_values)
        fmt = _pixel_format(px)
        t = self._bank(text_features)
        out, idx, prob = self._topk_out(px.shape[0], topk)
        self._in_chunks(px.shape[0], nb, lambda s, n: self._lib.mcm_score_topk(
            self._h, px[s:s + n].data_ptr(), fmt, int(x2), n, t.data_ptr(), t.shape[0], float(T), SCORE_KINDS[score], int(topk),
            out[s:s + n].data_ptr(), idx[s:s + n].data_ptr(), prob[s:s + n].data_ptr(), _stream_ptr()))
        return out, idx, prob

    def score_features(self, image_features, text_features, T: float = 1.0, score: str = "MCM", topk: int = 0,
                       tail: str = "lds", splits: int = 0, return_parts: bool = False):
        """features [b,P] + bank [K,P] → scores [b] fp32 on the device.  `topk` > 0 (at most 8): also which concepts
        matched — returns (scores, idx [b,topk] int32, prob [b,topk] fp32): the bank rows of the topk largest
        similarities (value descending, ties to the lower row, NaN never, -1 where nothing is left) and their
        softmax(sim / T); the scores are the bits of the `topk=0` call (include/mcm.h mcm_score_features_topk).
        `tail`: "lds" = the tail that keeps an image's K similarities in LDS and refuses (P + K) * 4 > 150 KiB; "stream" = the
        streamed tail (include/mcm_score_stream.h mcm_score_features_stream), any K; "auto" = "lds" wherever it takes the
        shape, "stream" exactly where it refuses.  The default here is "lds": this call's refusal of a bank past that size is
        part of its contract (tests/test_gpu_error_budget.py holds it); `score_images` / `score_images_x2`, which everything
        in detection.py and refine.py goes through, default to "auto".  The streamed tail alone takes `splits` (0 = the library's choice, n = the
        bank in exactly n ranges: results agree across it to rounding and are the same bits for a fixed value) and
        `return_parts=True`, which appends parts [b,5], all five kinds in SCORE_KINDS order, to what is returned."""
        import torch

        f = image_features.to(device=self.device, dtype=torch.float32).contiguous()
        if f.dim() != 2 or f.shape[1] != self.geo.proj_dim:
            raise ValueError(f"image_features must be [b,{self.geo.proj_dim}], got {tuple(f.shape)}")
        t = self._bank(text_features)
        if self._streams(tail, t.shape[0], splits, return_parts):
            return self._score_stream(f, t, T, score, topk, splits, return_parts)
        if topk:
            out, idx, prob = self._topk_out(f.shape[0], topk)
            self._check(self._lib.mcm_score_features_topk(self._h, f.data_ptr(), f.shape[0], t.data_ptr(), t.shape[0],
                                                          float(T), SCORE_KINDS[score], int(topk), out.data_ptr(),
                                                          idx.data_ptr(), prob.data_ptr(), _stream_ptr()))
            return out, idx, prob
        out = torch.empty(f.shape[0], device=self.device, dtype=torch.float32)
        self._check(self._lib.mcm_score_features(self._h, f.data_ptr(), f.shape[0], t.data_ptr(),
                                                 t.shape[0], float(T), SCORE_KINDS[score],
                                                 out.data_ptr(), _stream_ptr()))
        return out

    def score_kinds(self, image_features, text_features, T: float = 1.0, splits: int = 0):
        """features [b,P] + bank [K,P] → [b,5] fp32: MCM, max-logit, energy, entropy and var (SCORE_KINDS order) from one walk
        of the bank by the streamed tail, at any K."""
        return self.score_features(image_features, text_features, T, "MCM", tail="stream", splits=splits, return_parts=True)[1]

    # -- the streamed tail of the MCM family (include/mcm_score_stream.h) ---------------------------------
    def _streams(self, tail, K, splits, return_parts) -> bool:
        """Whether a call goes to the streamed tail.  "auto" sends it there exactly where the LDS tail refuses the shape
        (csrc/score.hip score_shape_ok: (P + K) * 4 bytes of LDS above include/mcm.h MCM_SCORE_LDS_MAX_BYTES, 150 KiB)."""
        if tail not in ("auto", "lds", "stream"):
            raise ValueError(f"tail must be 'auto', 'lds' or 'stream', got {tail!r}")
        lds_max = abi.DEFINES["MCM_SCORE_LDS_MAX_BYTES"]
        stream = tail == "stream" or (tail == "auto" and (self.geo.proj_dim + int(K)) * 4 > lds_max)
        if not stream and (splits or return_parts):
            raise ValueError("splits and return_parts belong to the streamed tail: pass tail='stream'")
        return stream

    def _score_stream(self, f, t, T, score, topk, splits, return_parts, out=None):
        """The streamed tail over features f [b,P] and bank t [K,P] (both as the kernels read them).  Returns scores, or
        (scores, idx, prob) with topk > 0, with parts [b,5] appended where asked for.  The workspace is a buffer of this
        object that grows on demand; queries go through in blocks of at most 4096 rows."""
        if not getattr(self._lib, "_mcm_score_stream", False):  # the extension header's entries are bound where they are used
            abi.declare(self._lib, names=list(abi.EXTENSION_PROTOTYPES))
            self._lib._mcm_score_stream = True
        B, K, T, kind, topk, splits = int(f.shape[0]), int(t.shape[0]), float(T), SCORE_KINDS[score], int(topk), int(splits)
        if topk:
            scores, idx, prob = self._topk_out(B, topk)
        else:
            scores, idx, prob = self._empty(B) if out is None else out, None, None
        parts = self._empty(B, 5, when=return_parts)
        self._bank_score(
            "score_features (streamed tail)", "_score_stream_work", B,
            lambda n: self._rules(B=n, T=T, splits=splits) + [
                (f"K={K} (1 <= K <= 2^31 - 1)", not 1 <= K <= 2 ** 31 - 1),
                (f"topk={topk} (0 <= topk <= {TOPK_MAX})", not 0 <= topk <= TOPK_MAX)],
            lambda n, need: self._lib.mcm_score_stream_workspace_bytes(self._h, n, K, topk, splits, need),
            lambda s, n, work: self._lib.mcm_score_features_stream(
                self._h, f[s:s + n].data_ptr(), n, t.data_ptr(), K, T, kind, topk, splits, work.data_ptr(), work.numel() * 4,
                scores[s:s + n].data_ptr(), _at(parts, s, n), _at(idx, s, n), _at(prob, s, n), _stream_ptr()))
        res = (scores, idx, prob) if topk else (scores,)
        res = res + (parts,) if return_parts else res
        return res if len(res) > 1 else res[0]

    def _score_images_stream(self, pixel_values, t, T, score, out, topk, x2, splits, return_parts):
        """`score_images` / `score_images_x2` by the streamed tail: `get_image_features(normalize=True)` of the arm into a
        buffer of this object that grows on demand, then `_score_stream` on it — the bits of
        `score_features(get_image_features(pixel_values, normalize=True), ..., tail="stream")`."""
        if x2:
            self._x2_batch()
        px = self._pixels(pixel_values)
        b = px.shape[0]
        feat = getattr(self, "_score_stream_feat", None)
        if feat is None or feat.shape[0] < b:
            feat = self._score_stream_feat = self._empty(b, self.geo.proj_dim)
        self._encode_into(px, feat[:b], True, x2)
        return self._score_stream(feat[:b], t, T, score, topk, splits, return_parts, out=out)

    def _score_images(self, pixel_values, text_features, T, score, out, topk, tail, splits, return_parts, x2: bool):
        """The body of `score_images` (x2 false) and `score_images_x2` (x2 true), and the one place that decides which entry a
        call takes: the image tower followed by the streamed tail where `_streams` says so, else mcm_score_topk with topk,
        else mcm_score_x2 on the split-activation arm, else mcm_score_u8 or mcm_score by the pixels' format."""
        t = self._bank(text_features)
        if self._streams(tail, t.shape[0], splits, return_parts):
            return self._score_images_stream(pixel_values, t, T, score, out, topk, x2, splits, return_parts)
        if topk:
            return self._score_images_topk(pixel_values, text_features, T, score, topk, x2=x2)
        nb = self._x2_batch() if x2 else self.max_batch
        px = self._pixels(pixel_values)
        fmt = _pixel_format(px)
        if x2:
            entry, form = self._lib.mcm_score_x2, (fmt,)
        else:  # the handle's own arm has one entry per pixel format
            entry, form = self._lib.mcm_score_u8 if fmt == abi.DEFINES["MCM_PIXELS_U8_NHWC"] else self._lib.mcm_score, ()
        if out is None:
            out = self._empty(px.shape[0])
        self._in_chunks(px.shape[0], nb, lambda s, n: entry(
            self._h, px[s:s + n].data_ptr(), *form, n, t.data_ptr(), t.shape[0], float(T), SCORE_KINDS[score],
            out[s:s + n].data_ptr(), _stream_ptr()))
        return out

    def score_images(self, pixel_values, text_features, T: float = 1.0, score: str = "MCM", out=None, topk: int = 0,
                     tail: str = "auto", splits: int = 0, return_parts: bool = False):
        """pixels [b,3,S,S] + pre-encoded bank [K,P] → scores [b] fp32 on device (one
        iteration of the reference loop, utils/detection_util.py:223-248).  `topk` > 0: (scores, idx, prob) as
        `score_features` returns them (`out` is not used then).  `tail`, `splits`, `return_parts`: as `score_features`; past
        the LDS tail's bank size the call is the image tower followed by the streamed tail."""
        return self._score_images(pixel_values, text_features, T, score, out, topk, tail, splits, return_parts, self.x2_default)

    # -- split-activation arm: the re-scorer of threshold refinement (include/mcm.h mcm_score_x2) ----------------------
    @property
    def x2_max_batch(self) -> int:
        """Largest batch of the split-activation arm on this handle's workspace (0: not an fp16 handle, or created without it)."""
        return int(self._lib.mcm_x2_max_batch(self._h))

    @property
    def kernel_faults(self) -> int:
        """Non-zero when a persistent kernel gave up a bounded wait (include/mcm.h mcm_kernel_faults): 0 in every correct run."""
        return int(self._lib.mcm_kernel_faults(self._h))

    def score_images_x2(self, pixel_values, text_features, T: float = 1.0, score: str = "MCM", out=None, topk: int = 0,
                        tail: str = "auto", splits: int = 0, return_parts: bool = False):
        """`score_images` through the split-activation arm: the same weights and workspace, every MFMA operand activation as a
        hi + lo pair of fp16 numbers — scores that agree with the exact-fp32 arm to fp32 round-off, at several times its
        speed.  Any number of images (chunks of `x2_max_batch`).  `topk` > 0: (scores, idx, prob), as `score_images`;
        `tail`, `splits`, `return_parts` too."""
        return self._score_images(pixel_values, text_features, T, score, out, topk, tail, splits, return_parts, True)

    def get_image_features_x2(self, pixel_values, normalize: bool = False):
        """`get_image_features` through the split-activation arm (raw projected features unless `normalize`)."""
        self._x2_batch()
        px = self._pixels(pixel_values)
        return self._encode_into(px, self._empty(px.shape[0], self.geo.proj_dim), normalize, x2=True)

    def x2_scorer(self):
        """An object with this scorer's `score_images` signature that runs the split-activation arm (mcm_amd.refine.Rescorer)."""
        return _X2Scorer(self)

    def reduce_bank(self, text_features, K: int, T: int):
        """[K*T,P] unit-norm template features (class-major) → [K,P] ensemble bank."""
        import torch

        f = text_features.to(device=self.device, dtype=torch.float32).contiguous()
        assert f.shape[0] == K * T
        out = torch.empty((K, self.geo.proj_dim), device=self.device, dtype=torch.float32)
        self._check(self._lib.mcm_reduce_bank(self._h, f.data_ptr(), K, T, out.data_ptr(), _stream_ptr()))
        return out

    def resize_crop(self, images):
        """Resize(S) + CenterCrop(S) of the reference's loader transform (utils/train_eval_util.py:27-33)
        on the device: `images` = sequence of uint8 [H_i, W_i, 3] RGB tensors → uint8 [B, S, S, 3], the
        input layout of `score_images` / `get_image_features`.  Bit-exact against Pillow."""
        import torch

        imgs = [im.to(device=self.device, dtype=torch.uint8).contiguous() for im in images]
        B, S = len(imgs), self.geo.image_size
        for im in imgs:
            if im.dim() != 3 or im.shape[2] != 3:
                raise ValueError("images must be uint8 [H, W, 3] RGB")
        ptrs = (ctypes.c_void_p * B)(*[im.data_ptr() for im in imgs])
        hs = (ctypes.c_int32 * B)(*[im.shape[0] for im in imgs])
        ws = (ctypes.c_int32 * B)(*[im.shape[1] for im in imgs])
        out = torch.empty((B, S, S, 3), device=self.device, dtype=torch.uint8)
        self._check(self._lib.mcm_resize_crop_u8(self._h, ptrs, hs, ws, B, out.data_ptr(), _stream_ptr()))
        return out

    def resize_crop_packed(self, packed, offsets, heights, widths, out=None):
        """`resize_crop` over images that already sit back to back in ONE device buffer (`packed`: uint8 1-D device
        tensor; image i = [heights[i], widths[i], 3] at byte offset offsets[i]) — what mcm_amd.ingest.PackedImagePipe
        uploads with one copy per batch.  Asynchronous on the current stream."""
        import torch

        B, S = len(offsets), self.geo.image_size
        if packed.dtype != torch.uint8 or not packed.is_cuda:
            raise ValueError("packed must be a uint8 device tensor")
        base = packed.data_ptr()
        ptrs = (ctypes.c_void_p * B)(*[base + int(o) for o in offsets])
        hs = (ctypes.c_int32 * B)(*[int(v) for v in heights])
        ws = (ctypes.c_int32 * B)(*[int(v) for v in widths])
        if out is None:
            out = torch.empty((B, S, S, 3), device=self.device, dtype=torch.uint8)
        self._check(self._lib.mcm_resize_crop_u8(self._h, ptrs, hs, ws, B, out.data_ptr(), _stream_ptr()))
        return out

    def jpeg_reconstruct(self, coef_dev, meta, quant, n: int, rgb_dev, rgb_offsets):
        """Device half of the JPEG ingest (mcm_jpeg_reconstruct): the coefficients mcm_jpeg_entropy_decode wrote (device
        copy `coef_dev`, uint8 1-D) -> RGB uint8 [H_i, W_i, 3] at rgb_dev + rgb_offsets[i], byte for byte Pillow's decode.
        `meta`: ctypes array of config.JpegImage, `quant`: uint16 numpy [n, 3, 64] (both as the entropy decoder filled them);
        images whose status is not 0 are skipped.  Asynchronous on the current stream."""
        offs = (ctypes.c_int64 * n)(*[int(o) for o in rgb_offsets])
        self._check(self._lib.mcm_jpeg_reconstruct(self._h, coef_dev.data_ptr(), ctypes.addressof(meta), quant.ctypes.data, n,
                                                   rgb_dev.data_ptr(), offs, _stream_ptr()))

    def measures(self, pos_scores, neg_scores, recall_level: float = 0.95, negate: bool = False):
        """`get_measures` (reference utils/detection_util.py:108-119) on device score vectors:
        (auroc, aupr, fpr) with ID = positive class; `negate=True` evaluates on -score, which is
        how `get_and_print_results` (:255) calls it."""
        import torch

        pos = pos_scores.to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
        neg = neg_scores.to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
        out = (ctypes.c_double * 3)()
        self._check(self._lib.mcm_measures(self._h, pos.data_ptr(), pos.numel(), neg.data_ptr(),
                                           neg.numel(), int(negate), float(recall_level), out,
                                           _stream_ptr()))
        return float(out[0]), float(out[1]), float(out[2])

    def histogram(self, scores, edges):
        """numpy.histogram(scores, edges)[0] on the device → int64 tensor [len(edges)-1]."""
        import torch

        x = scores.to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
        e = torch.as_tensor(edges, dtype=torch.float32).to(self.device).contiguous()
        out = torch.empty(e.numel() - 1, device=self.device, dtype=torch.int64)
        self._check(self._lib.mcm_score_histogram(self._h, x.data_ptr(), x.numel(), e.data_ptr(),
                                                  e.numel() - 1, out.data_ptr(), _stream_ptr()))
        return out

    # -- fp16 saturation watch ---------------------------------------------------------------
    def saturation_count(self, reset: bool = True) -> int:
        """Waves that packed an fp16 activation at the saturation value (±65504) since the last reset, over
        every call on this handle; 0 = nothing left the fp16 range.  Always 0 in bf16 / fp32 mode."""
        out = ctypes.c_uint64(0)
        self._check(self._lib.mcm_saturation_count(self._h, int(reset), ctypes.byref(out), _stream_ptr()))
        return int(out.value)

    def saturation_check(self, on: bool):
        self._check(self._lib.mcm_saturation_check(self._h, int(on)))

    def warn_if_saturated(self, what: str = "") -> int:
        """RuntimeWarning when any fp16 activation saturated since the last call (the CLI calls this per set)."""
        n = self.saturation_count(reset=True)
        if n:
            import warnings

            warnings.warn(f"fp16 activations saturated at +-65504 in {n} wave(s){' while scoring ' + what if what else ''}: "
                          "those elements lost precision (outlier channels?) — rerun with --dtype bf16 or fp32 to compare",
                          RuntimeWarning, stacklevel=2)
        return n

    # -- per-kernel timing -------------------------------------------------------------------
    def profile(self, on: bool):
        self._check(self._lib.mcm_profile_enable(self._h, int(on)))

    def profile_read(self) -> Dict[str, Dict[str, float]]:
        n = len(KERNEL_CLASSES)
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_int64 * n)()
        fl = (ctypes.c_double * n)()
        self._check(self._lib.mcm_profile_read(self._h, ms, cnt, fl))
        return {k: {"ms": ms[i], "launches": int(cnt[i]), "flops": fl[i]}
                for i, k in enumerate(KERNEL_CLASSES)}


class _X2Scorer:
    """`NativeCLIP.x2_scorer()`: the split-activation arm behind the `score_images` / `max_batch` / `device` surface
    mcm_amd.refine.Rescorer drives."""

    label = "split-activation fp16 arm of the same handle (mcm_score_x2)"

    def __init__(self, net):
        self.net, self.device, self.geo = net, net.device, net.geo
        self.max_batch = net.x2_max_batch

    def score_images(self, pixel_values, text_features, T: float = 1.0, score: str = "MCM", out=None, topk: int = 0,
                     tail: str = "auto"):
        return self.net.score_images_x2(pixel_values, text_features, T, score, out=out, topk=topk, tail=tail)


class GraphedScorer:
    """One iteration of the hot loop — `net.score_images(pixels, bank, T, score)` — captured once into a hipGraph and
    replayed: for SMALL batches the ~110 kernel launches of a step cost more host time than the kernels take on the device
    (batch 8 at B/16: 1.4 ms per step eager), a replay is one launch.  The C ABI allocates nothing after `mcm_create`, so the
    call is capturable as it is (include/mcm.h).  The graph holds the pointers it was captured with: `pixels` are copied
    into its static input (device to device) unless the caller fills `scorer.input` itself, the scores land in
    `scorer.output` (valid until the next call).  Per-kernel profiling must be off while capturing.

        scorer = GraphedScorer(net, batch=8, bank=bank)          # capture (one warm-up call + capture)
        scores = scorer(pixels)                                   # replay; same bits as net.score_images(pixels, bank)
    """

    def __init__(self, net: "NativeCLIP", batch: int, bank, T: float = 1.0, score: str = "MCM", uint8: bool = False,
                 input=None):
        import torch

        S = net.geo.image_size
        self.net, self.batch = net, int(batch)
        self.bank = net._bank(bank)
        if input is not None:  # capture on the caller's own static buffer (no copy per call)
            self.input = net._pixels(input)
            if self.input.data_ptr() != input.data_ptr() or self.input.shape[0] != self.batch:
                raise ValueError("input must be a contiguous device tensor of the captured batch size")
        else:
            self.input = (torch.zeros((self.batch, S, S, 3), dtype=torch.uint8, device=net.device) if uint8
                          else torch.zeros((self.batch, 3, S, S), dtype=torch.float32, device=net.device))
        self.output = torch.empty(self.batch, dtype=torch.float32, device=net.device)
        self._stream = torch.cuda.Stream(device=net.device)
        self._stream.wait_stream(torch.cuda.current_stream(net.device))
        with torch.cuda.stream(self._stream):  # first launches set kernel attributes: outside the capture
            net.score_images(self.input, self.bank, T, score, out=self.output)
        self._stream.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self._stream):
            net.score_images(self.input, self.bank, T, score, out=self.output)

    def __call__(self, pixel_values=None):
        if pixel_values is not None:
            if tuple(pixel_values.shape) != tuple(self.input.shape) or pixel_values.dtype != self.input.dtype:
                raise ValueError(f"the graph was captured for {tuple(self.input.shape)} {self.input.dtype}")
            self.input.copy_(pixel_values, non_blocking=True)
        self.graph.replay()
        return self.output


def build_model(ckpt: str = "ViT-B/16", *, weights: Optional[str] = None, seed: int = 0,
                synthetic_regime: str = "fp16-exact", **kw) -> NativeCLIP:
    """`set_model_clip` counterpart (reference utils/train_eval_util.py:15-36): checkpoint
    name → NativeCLIP.  `weights` = path to a real checkpoint; default = seeded synthetic
    parameters (no checkpoint exists offline), by default rounded to fp16 values like the reference's
    checkpoints are (`synthetic_regime="fp32"`: as drawn — a 16-bit arm then runs the split-weight GEMMs)."""
    from .weights import load_state_dict_file, synth_state_dict

    geo = geometry(ckpt)
    sd = load_state_dict_file(weights, geo) if weights else synth_state_dict(geo, seed, synthetic_regime)
    return NativeCLIP(geo, sd, synthetic_weights=not weights, **kw)
