"""LPIPS on the HIP path (csrc/lpips.hip, include/mobgs_hip.h K24): the "net-lin" model with the AlexNet trunk, version
0.1 -- the spatial average the reference's metrics.py:84-85, :127-131 and eval.py:76 evaluate, the per-pixel map of
spatial=True and the two masked averages (the reference's mask=, dycheck's compute_lpips) -- for a whole batch of image
pairs in one call, without the reference's models/ package, torchvision or a DataParallel wrapper.

    model = LpipsAlex.from_files(trunk="alexnet-owt-7be5be79.pth", heads=".../models/weights/v0.1/alex.pth", device="cuda")
    model = LpipsAlex(trunk_state_dict, heads_state_dict, device="cuda")
    r = model(pred, gt, clamp=False, quantize=False)   # [B,3,H,W] in [0, 1] -> LpipsResult(total [B], per_layer [B,5]) float64
    v = model.forward(in0, in1)                         # the reference's call: inputs in [-1, 1] -> [B,1,1,1] fp32
    maps = model.features(img)                          # the five ReLU maps, NCHW, for tests and debugging
    s = model.spatial(pred, gt, mask)                   # LpipsSpatial: map [B,1,H,W] fp32, mean, masked_mean, ... float64
    m = model.forward_spatial(in0, in1)                 # PerceptualLoss(spatial=True).forward: [B,1,H,W] fp32
    v = model.forward_masked(in0, in1, mask)            # PNetLin.forward(mask=): a 0-dim fp32 tensor
    l = model.loss(pred, gt, clamp=False, normalize=True)   # [B] fp32 WITH a gradient for pred and / or gt (a training loss)

mirrors /root/reference/models/networks_basic.py:16-28 and :68-105 (spatial_average, upsample, PNetLin.forward,
ScalingLayer), models/pretrained_networks.py:57-95 (the five slices of torchvision's alexnet().features),
models/__init__.py:26-44, metrics.py:49-51 and dycheck_metrics.py:203-244.  Everything but loss() is forward only, under
no_grad; tensors must live on a HIP device.

THE LOSS (utils/loss_utils.py:228-230 of the reference, mobgs_amd.loss_utils.lpips_loss here): loss() is an autograd
function over mobgs_lpips_alex (which stores the five ReLU maps) and mobgs_lpips_alex_bwd -- the distance heads' backward,
the backward-data pass of layers 5 .. 2 on the forward's GEMM body, max-pool backward as a gather, the first layer into the
image.  Its value has the bits of model(pred, gt).total.float(); the gradient goes to whichever of pred / gt requires one,
only those images are walked, and it is bit-identical from run to run, whatever the batch and the chunking, and exactly
+0 for equal images.  Two deliberate conventions: where a feature vector is all zero the reference's autograd
gives NaN (the derivative of sqrt at 0 times 0); here that pixel's gradient is 0.  Max-pool ties go to the first maximum in
row-major order of the window, torch's rule.  The trunk and the heads are constants: they get no gradient.

THE MAP is defined at H x W for every size: bilinear, align_corners=False, with the scale h / H (nn.Upsample(size=)).  The
reference passes scale_factor = H / h, for which torch sizes the output as floor(h * scale_factor): H - 1 for some sizes
(H = 49 with h = 11, 61 with 14, 98 with 11, ...), where the reference raises.  Where the reference's form works the two
agree to rounding.

THE WEIGHTS are the caller's: torchvision's AlexNet file for the trunk (keys features.{0,3,6,8,10}.{weight,bias}; other keys,
the classifier's, are ignored) and the reference's v0.1/alex.pth for the heads (keys lin{0..4}.model.1.weight).  They are
packed once, at construction, into the K-major layout the convolution kernel reads.  The value a user compares with the
published one rests on that trunk file (README, "UNPINNED").

Not here: the VGG and SqueezeNet trunks, gradients of the spatial map and of the masked forms, gradients with respect to the
trunk or the heads, reduced precision.  forward() itself keeps refusing mask= and
spatial=True (NotImplementedError): forward_masked and forward_spatial are those calls.
"""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Optional

import torch

from . import _lib
from ._lib import check, device_tensor, f32c, ptr, stream

CIN, COUT = (3, 64, 192, 384, 256), (64, 192, 384, 256, 256)
KS, STRIDE, PAD = (11, 5, 3, 3, 3), (4, 1, 1, 1, 1), (2, 2, 1, 1, 1)
TRUNK_INDEX = (0, 3, 6, 8, 10)                      # the convolutions inside torchvision's alexnet().features
K_STEP = 32                                          # the kernel's K step; mobgs_lpips_pack_k answers with it (tested)
MIN_EDGE = 31
UNIT_RANGE, CLAMP, QUANTIZE = (_lib._DEFINES[k] for k in ("MOBGS_LPIPS_UNIT_RANGE", "MOBGS_LPIPS_CLAMP",
                                                           "MOBGS_LPIPS_QUANTIZE"))
COLUMNS = _lib._DEFINES["MOBGS_LPIPS_COLUMNS"]
SPATIAL_COLUMNS = _lib._DEFINES["MOBGS_LPIPS_SPATIAL_COLUMNS"]


class LpipsResult(NamedTuple):
    total: torch.Tensor          # [B] float64, device: the sum of the five layer values
    per_layer: torch.Tensor      # [B,5] float64, device


class LpipsSpatial(NamedTuple):
    """LpipsAlex.spatial: float64 device tensors per pair (include/mobgs_hip.h K24, the spatial row), and the map."""
    map: Optional[torch.Tensor]      # [B,1,H,W] fp32: the sum of the five upsampled distance maps; None without want_map
    mean: torch.Tensor               # [B]: the map's mean
    masked_mean: torch.Tensor        # [B]: dycheck's masked_mean, sum(map m) / max(sum(m), 1e-6)
    masked_total: torch.Tensor       # [B]: the sum of masked_per_layer
    masked_per_layer: torch.Tensor   # [B,5]: the reference's masked average per pair, numerators / (denominators + 1e-8)
    numerators: torch.Tensor         # [B,5]: sum(d_l m_l), m_l the mask resized to the tap by nearest neighbour
    denominators: torch.Tensor       # [B,5]: sum(m_l)
    map_mask_sum: torch.Tensor       # [B]: sum(map m), sum(m) and sum(map)
    mask_sum: torch.Tensor
    map_sum: torch.Tensor


def pack_k(layer: int) -> int:
    """Rows of layer `layer`'s packed weight (1 .. 5): Cin k k rounded up to the kernel's K step."""
    K = CIN[layer - 1] * KS[layer - 1] ** 2
    return (K + K_STEP - 1) // K_STEP * K_STEP


def tap_sizes(H: int, W: int) -> List[tuple]:
    """(h, w) of the five ReLU maps of an H x W image; ValueError below 31, where the second pool has no output."""
    if H < MIN_EDGE or W < MIN_EDGE:
        raise ValueError(f"LPIPS (AlexNet): H, W >= {MIN_EDGE} (the second max-pool has no output below), got {H} x {W}")
    def pool(n):
        return (n - 3) // 2 + 1
    h1, w1 = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    h2, w2 = pool(h1), pool(w1)
    h3, w3 = pool(h2), pool(w2)
    return [(h1, w1), (h2, w2), (h3, w3), (h3, w3), (h3, w3)]


def pack_conv_weight(weight: torch.Tensor, layer: int) -> torch.Tensor:
    """[Cout, Cin, k, k] -> [Kpad, Cout], the layout of include/mobgs_hip.h K24: row (ky k + kx) Cin + ci for layers 2 .. 5,
    row (ci 11 + ky) 11 + kx for layer 1, zero rows up to pack_k(layer).  Plain torch, any device."""
    cout, cin, k = COUT[layer - 1], CIN[layer - 1], KS[layer - 1]
    if tuple(weight.shape) != (cout, cin, k, k):
        raise ValueError(f"pack_conv_weight: layer {layer} needs [{cout}, {cin}, {k}, {k}], got {tuple(weight.shape)}")
    rows = weight.reshape(cout, -1).t() if layer == 1 else weight.permute(2, 3, 1, 0).reshape(-1, cout)
    packed = weight.new_zeros(pack_k(layer), cout)
    packed[:rows.shape[0]] = rows
    return packed.contiguous()


def bwd_pack_k(layer: int) -> int:
    """Rows of layer `layer`'s weight packed for the backward-data pass (2 .. 5): Cout k k, a multiple of the K step."""
    return COUT[layer - 1] * KS[layer - 1] ** 2


def pack_conv_weight_bwd(weight: torch.Tensor, layer: int) -> torch.Tensor:
    """[Cout, Cin, k, k] -> [Cout k k, Cin] for the backward-data pass of layers 2 .. 5 (include/mobgs_hip.h K24, backward):
    row (ky k + kx) Cout + co holds weight[co, ci, k - 1 - ky, k - 1 - kx] in column ci.  Plain torch, any device."""
    cout, cin, k = COUT[layer - 1], CIN[layer - 1], KS[layer - 1]
    if layer < 2 or tuple(weight.shape) != (cout, cin, k, k):
        raise ValueError(f"pack_conv_weight_bwd: layer {layer} (2 .. 5) needs [{cout}, {cin}, {k}, {k}], got "
                         f"{tuple(weight.shape)}")
    return weight.flip(2, 3).permute(2, 3, 0, 1).reshape(-1, cin).contiguous()


def unpack_conv_weight(packed: torch.Tensor, layer: int) -> torch.Tensor:
    """The inverse of pack_conv_weight (the padding rows are dropped)."""
    cout, cin, k = COUT[layer - 1], CIN[layer - 1], KS[layer - 1]
    rows = packed[:cin * k * k]
    if layer == 1:
        return rows.t().reshape(cout, cin, k, k).contiguous()
    return rows.reshape(k, k, cin, cout).permute(3, 2, 0, 1).contiguous()


def check_state_dicts(trunk, heads):
    """-> (five conv weights [Cout,Cin,k,k], five biases [Cout], five head vectors [Cout]), fp32 on the host.  A missing
    key, a wrong shape or a dtype that is no floating point raises ValueError naming the key."""
    def take(sd, key, shape, what):
        if not hasattr(sd, "keys") or key not in sd:
            raise ValueError(f"LpipsAlex: the {what} state dict has no key {key!r}")
        t = sd[key]
        if not torch.is_tensor(t):
            raise ValueError(f"LpipsAlex: {key!r} of the {what} state dict is no tensor")
        if tuple(t.shape) != shape:
            raise ValueError(f"LpipsAlex: {key!r} must be {list(shape)}, got {list(t.shape)}")
        if not t.dtype.is_floating_point:
            raise ValueError(f"LpipsAlex: {key!r} must be a floating-point tensor, got {t.dtype}")
        return t.detach().to("cpu", torch.float32)
    ws, bs, ls = [], [], []
    for l, idx in enumerate(TRUNK_INDEX):
        ws.append(take(trunk, f"features.{idx}.weight", (COUT[l], CIN[l], KS[l], KS[l]), "trunk"))
        bs.append(take(trunk, f"features.{idx}.bias", (COUT[l],), "trunk"))
        ls.append(take(heads, f"lin{l}.model.1.weight", (1, COUT[l], 1, 1), "heads").reshape(-1))
    return ws, bs, ls


def _flags(clamp, quantize) -> int:
    return UNIT_RANGE | (CLAMP if clamp else 0) | (QUANTIZE if quantize else 0)


def _pair(what, a, b):
    device_tensor(what, "the first image", a), device_tensor(what, "the second image", b)
    if a.dim() == 3:
        a = a[None]
    if b.dim() == 3:
        b = b[None]
    if a.dim() != 4 or a.shape[1] != 3 or a.shape != b.shape:
        raise ValueError(f"{what}: both images must be [B,3,H,W], got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.shape[0] < 1:
        raise ValueError(f"{what}: an empty batch")
    tap_sizes(a.shape[2], a.shape[3])
    return f32c(a.detach()), f32c(b.detach())


def _mask(what, mask, like):
    """None, [B,H,W], [B,C,H,W] (its first channel, as the reference's mask[:, 0:1]) or, for one pair, [H,W] -> None or
    [B,H,W] fp32 contiguous on the images' device."""
    if mask is None:
        return None
    device_tensor(what, "the mask", mask)
    B, _, H, W = like.shape
    if mask.dim() == 4:
        mask = mask[:, 0]
    elif mask.dim() == 2:
        mask = mask[None]
    if mask.dim() != 3 or tuple(mask.shape) != (B, H, W):
        raise ValueError(f"{what}: the mask must be [B,H,W] or [B,C,H,W] with B, H, W = {B}, {H}, {W}, got "
                         f"{tuple(mask.shape)}")
    if mask.device != like.device:
        raise ValueError(f"{what}: the mask is on {mask.device}, the images on {like.device}")
    return f32c(mask.detach())


class _LpipsLoss(torch.autograd.Function):
    """img0, img1 [B,3,H,W] fp32 contiguous -> the totals [B] fp32.  The forward keeps the five ReLU maps of all images."""

    @staticmethod
    def forward(ctx, img0, img1, model, flags):
        a, b = img0.detach(), img1.detach()
        out, taps, chunk = model._loss_forward(a, b, flags)
        ctx.model, ctx.flags, ctx.chunk = model, flags, chunk
        ctx.save_for_backward(a, b, *taps)
        return out[:, 0].float()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v_total):
        a, b, *taps = ctx.saved_tensors
        want0, want1 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want0 or want1):
            return None, None, None, None
        g0, g1, _ = ctx.model._loss_backward(a, b, ctx.flags, taps, f32c(v_total), want0, want1, chunk=ctx.chunk)
        return g0, g1, None, None


class LpipsAlex:
    """The model, with its weights packed on one device.  Calls run on the current stream with 13 launches per chunk, no
    synchronisation, no read-back and no allocation that depends on the data: they can be recorded into a graph.  A pair's
    result is bit-identical from run to run, whatever the batch around it, and exactly 0 for equal images."""

    max_scratch_bytes = 1 << 30      # scratch budget per call: a batch whose scratch exceeds it is processed in chunks

    def __init__(self, trunk_state_dict, heads_state_dict, device="cuda"):
        ws, bs, ls = check_state_dicts(trunk_state_dict, heads_state_dict)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("LpipsAlex: device must be a HIP device (device='cuda'); there is no CPU path")
        lib = _lib.load()
        for l in range(5):
            if int(lib.mobgs_lpips_pack_k(l + 1)) != pack_k(l + 1):
                raise RuntimeError(f"LpipsAlex: the library packs layer {l + 1} to {lib.mobgs_lpips_pack_k(l + 1)} rows, "
                                   f"this module to {pack_k(l + 1)}")
        self.weights = [pack_conv_weight(w, l + 1).to(self.device) for l, w in enumerate(ws)]
        self.biases = [b.contiguous().to(self.device) for b in bs]
        self.heads = [v.contiguous().to(self.device) for v in ls]
        fields = {}
        for l in range(5):
            fields[f"w{l + 1}"] = self.weights[l].data_ptr()
            fields[f"b{l + 1}"] = self.biases[l].data_ptr()
            fields[f"lin{l + 1}"] = self.heads[l].data_ptr()
        self._record = _lib.MobgsLpipsWeights(**fields)
        for l in range(2, 6):
            if int(lib.mobgs_lpips_bwd_pack_k(l)) != bwd_pack_k(l) or bwd_pack_k(l) % K_STEP:
                raise RuntimeError(f"LpipsAlex: the library packs layer {l}'s backward weight to "
                                   f"{lib.mobgs_lpips_bwd_pack_k(l)} rows, this module to {bwd_pack_k(l)}")
        self.bwd_weights = [pack_conv_weight_bwd(ws[l - 1], l).to(self.device) for l in range(2, 6)]
        self._bwd_record = _lib.MobgsLpipsBwdWeights(**{f"w{l}": self.bwd_weights[l - 2].data_ptr() for l in range(2, 6)})

    @classmethod
    def from_files(cls, trunk, heads, device="cuda"):
        """trunk: torchvision's alexnet-owt-7be5be79.pth; heads: the reference's models/weights/v0.1/alex.pth."""
        return cls(torch.load(trunk, map_location="cpu"), torch.load(heads, map_location="cpu"), device=device)

    # ---- the call -----------------------------------------------------------------------------------------------------

    def _chunk(self, B, H, W, spatial=False):
        """The largest number of pairs whose scratch fits max_scratch_bytes (at least one)."""
        lib = _lib.load()
        query = lib.mobgs_lpips_spatial_scratch_bytes if spatial else lib.mobgs_lpips_scratch_bytes
        n = B
        while n > 1 and int(query(n, H, W)) > self.max_scratch_bytes:
            n = (n + 1) // 2
        if int(query(n, H, W)) == 0:
            raise ValueError(f"LpipsAlex: B = {n}, H = {H}, W = {W} is outside what mobgs_lpips_alex accepts")
        return n

    def _run(self, img0, img1, flags, taps=None):
        lib = _lib.load()
        B, _, H, W = img0.shape
        dev = img0.device
        out = torch.empty(B, COLUMNS, dtype=torch.float64, device=dev)
        n = B if taps is not None else self._chunk(B, H, W)
        nbytes = int(lib.mobgs_lpips_scratch_bytes(n, H, W))
        if nbytes == 0:
            raise ValueError(f"LpipsAlex: B = {n}, H = {H}, W = {W} is outside what mobgs_lpips_alex accepts")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        tap_ptrs = None
        if taps is not None:
            tap_ptrs = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in taps])
        with torch.cuda.device(dev):
            for b0 in range(0, B, n):
                b1 = min(B, b0 + n)
                check(lib.mobgs_lpips_alex(b1 - b0, H, W, ptr(img0[b0:b1]), ptr(img1[b0:b1]), ctypes.byref(self._record),
                                           flags, ptr(scratch), nbytes, ptr(out[b0:b1]), tap_ptrs, stream()),
                      "mobgs_lpips_alex")
        return out

    # ---- the loss: forward with the taps kept, backward through mobgs_lpips_alex_bwd --------------------------------------

    def _loss_chunk(self, B, H, W):
        """The largest number of pairs whose scratch (the larger of the two calls') and taps fit max_scratch_bytes."""
        lib = _lib.load()
        per_pair = 2 * 4 * sum(h * w * c for (h, w), c in zip(tap_sizes(H, W), COUT))
        def need(n):
            return max(int(lib.mobgs_lpips_scratch_bytes(n, H, W)), int(lib.mobgs_lpips_bwd_scratch_bytes(n, H, W))) + \
                n * per_pair
        n = B
        while n > 1 and need(n) > self.max_scratch_bytes:
            n = (n + 1) // 2
        if int(lib.mobgs_lpips_bwd_scratch_bytes(n, H, W)) == 0:
            raise ValueError(f"LpipsAlex: B = {n}, H = {H}, W = {W} is outside what mobgs_lpips_alex accepts")
        return n

    def _loss_forward(self, img0, img1, flags):
        """-> (out [B, COLUMNS] float64, the five taps [2B,h,w,C] of the whole batch, the chunk), chunked like _run."""
        lib = _lib.load()
        B, _, H, W = img0.shape
        dev = img0.device
        n = self._loss_chunk(B, H, W)
        out = torch.empty(B, COLUMNS, dtype=torch.float64, device=dev)
        taps = [torch.empty(2 * B, h, w, c, dtype=torch.float32, device=dev) for (h, w), c in zip(tap_sizes(H, W), COUT)]
        nbytes = int(lib.mobgs_lpips_scratch_bytes(n, H, W))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            for b0 in range(0, B, n):
                b1 = min(B, b0 + n)
                tap_ptrs = (ctypes.c_void_p * 5)(*[t[2 * b0:2 * b1].data_ptr() for t in taps])
                check(lib.mobgs_lpips_alex(b1 - b0, H, W, ptr(img0[b0:b1]), ptr(img1[b0:b1]), ctypes.byref(self._record),
                                           flags, ptr(scratch), nbytes, ptr(out[b0:b1]), tap_ptrs, stream()),
                      "mobgs_lpips_alex")
        return out, taps, n

    def _loss_backward(self, img0, img1, flags, taps, v_total, want0, want1, chunk=None, want_tap_grads=False):
        """-> (g_img0, g_img1 [B,3,H,W] fp32 or None, tap gradients or None): one mobgs_lpips_alex_bwd call per chunk.  The
        tap gradients ([n B, h, w, C] channel-last, n wanted sides per pair) are for tests and debugging."""
        lib = _lib.load()
        B, _, H, W = img0.shape
        dev = img0.device
        n = chunk or self._loss_chunk(B, H, W)
        sides = int(want0) + int(want1)
        g0 = torch.empty_like(img0) if want0 else None
        g1 = torch.empty_like(img1) if want1 else None
        tg = None
        if want_tap_grads:
            tg = [torch.empty(sides * B, h, w, c, dtype=torch.float32, device=dev)
                  for (h, w), c in zip(tap_sizes(H, W), COUT)]
        nbytes = int(lib.mobgs_lpips_bwd_scratch_bytes(n, H, W))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            for b0 in range(0, B, n):
                b1 = min(B, b0 + n)
                tap_ptrs = (ctypes.c_void_p * 5)(*[t[2 * b0:2 * b1].data_ptr() for t in taps])
                tg_ptrs = None if tg is None else (ctypes.c_void_p * 5)(*[t[sides * b0:sides * b1].data_ptr() for t in tg])
                check(lib.mobgs_lpips_alex_bwd(b1 - b0, H, W, ptr(img0[b0:b1]), ptr(img1[b0:b1]),
                                               ctypes.byref(self._record), ctypes.byref(self._bwd_record), flags, tap_ptrs,
                                               ptr(v_total[b0:b1]), ptr(scratch), nbytes,
                                               ptr(None if g0 is None else g0[b0:b1]),
                                               ptr(None if g1 is None else g1[b0:b1]), tg_ptrs, stream()),
                      "mobgs_lpips_alex_bwd")
        return g0, g1, tg

    def loss(self, pred, gt, *, clamp=False, normalize=True) -> torch.Tensor:
        """LPIPS as a training loss: pred, gt [B,3,H,W] (or [3,H,W]) in [0, 1] (normalize=False: in [-1, 1], as
        PerceptualLoss.forward takes them) -> [B] fp32 with the bits of self(pred, gt, clamp=clamp).total.float(), and a
        gradient for whichever of pred / gt requires one.  clamp: both are clamped to [0, 1] first; the gradient passes
        where 0 <= value <= 1.  There is no quantize here: the 8-bit truncation has no gradient.  13 launches forward, 12 or
        13 backward per chunk, no synchronisation, no read-back, no allocation that depends on the data: a forward +
        backward can be recorded into a graph (GraphedCallable)."""
        device_tensor("LpipsAlex.loss", "the first image", pred), device_tensor("LpipsAlex.loss", "the second image", gt)
        p = pred[None] if pred.dim() == 3 else pred
        g = gt[None] if gt.dim() == 3 else gt
        _pair("LpipsAlex.loss", p, g)                    # the forward's checks
        flags = (UNIT_RANGE if normalize else 0) | (CLAMP if clamp else 0)
        return _LpipsLoss.apply(f32c(g), f32c(p), self, flags)   # the reference's order: ground truth first

    def _run_spatial(self, img0, img1, mask, flags, want_map):
        """-> (out [B, SPATIAL_COLUMNS] float64, map [B,1,H,W] fp32 or None), chunked like _run."""
        lib = _lib.load()
        B, _, H, W = img0.shape
        dev = img0.device
        out = torch.empty(B, SPATIAL_COLUMNS, dtype=torch.float64, device=dev)
        fmap = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev) if want_map else None
        n = self._chunk(B, H, W, spatial=True)
        nbytes = int(lib.mobgs_lpips_spatial_scratch_bytes(n, H, W))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            for b0 in range(0, B, n):
                b1 = min(B, b0 + n)
                check(lib.mobgs_lpips_alex_spatial(b1 - b0, H, W, ptr(img0[b0:b1]), ptr(img1[b0:b1]),
                                                   ctypes.byref(self._record), ptr(None if mask is None else mask[b0:b1]),
                                                   flags, ptr(scratch), nbytes, ptr(None if fmap is None else fmap[b0:b1]),
                                                   ptr(out[b0:b1]), stream()), "mobgs_lpips_alex_spatial")
        return out, fmap

    @torch.no_grad()
    def spatial(self, pred, gt, mask=None, *, clamp=False, quantize=False, want_map=True) -> LpipsSpatial:
        """pred, gt [B,3,H,W] (or [3,H,W]) in [0, 1]; mask [B,H,W] / [B,C,H,W] (first channel) in [0, 1], or None = all ones;
        clamp, quantize as in __call__.  The images are taken as given: dycheck's compute_lpips multiplies them by the mask
        first (mobgs_amd.metrics.compute_lpips does).  15 launches per chunk, no synchronisation, no read-back.  The row of
        a pair has the same bits with and without want_map, whatever the batch and the chunking."""
        p, g = _pair("LpipsAlex.spatial", pred, gt)
        m = _mask("LpipsAlex.spatial", mask, p)
        out, fmap = self._run_spatial(g, p, m, _flags(clamp, quantize), want_map)
        return LpipsSpatial(fmap, out[:, 0], out[:, 1], out[:, 5], out[:, 6:11], out[:, 11:16], out[:, 16:21], out[:, 2],
                            out[:, 3], out[:, 4])

    @torch.no_grad()
    def forward_spatial(self, pred, target, normalize=False) -> torch.Tensor:
        """PerceptualLoss(spatial=True).forward: inputs in [-1, 1] (normalize=True: in [0, 1]) -> the map [B,1,H,W] fp32,
        at H x W for every size (see the module docstring)."""
        a, b = _pair("LpipsAlex.forward_spatial", target, pred)
        return self._run_spatial(a, b, None, UNIT_RANGE if normalize else 0, True)[1]

    @torch.no_grad()
    def forward_masked(self, pred, target, mask, normalize=False) -> torch.Tensor:
        """PNetLin.forward(mask=) through PerceptualLoss.forward (spatial=False): per layer sum(d_l m_l) / (sum(m_l) + 1e-8)
        with BOTH sums taken over the whole batch, as the reference's torch.sum does, then the sum of the five -> a 0-dim
        fp32 tensor.  mask [B,C,H,W] (its first channel) or [B,H,W]."""
        a, b = _pair("LpipsAlex.forward_masked", target, pred)
        if mask is None:
            raise ValueError("LpipsAlex.forward_masked: a mask is required (forward() is the call without one)")
        m = _mask("LpipsAlex.forward_masked", mask, a)
        out, _ = self._run_spatial(a, b, m, UNIT_RANGE if normalize else 0, False)
        layers = out[:, 11:16].sum(0) / (out[:, 16:21].sum(0) + 1e-8)
        return layers.sum().float()

    @torch.no_grad()
    def __call__(self, pred, gt, clamp=False, quantize=False) -> LpipsResult:
        """pred, gt [B,3,H,W] (or [3,H,W]) in [0, 1].  clamp: both are clamped to [0, 1] first; quantize: the prediction is
        then replaced by floor(clip(pred, 0, 1) * 255) / 255 (eval.py:162): the score of the written PNG."""
        p, g = _pair("LpipsAlex", pred, gt)
        out = self._run(g, p, _flags(clamp, quantize))    # the reference's order (metrics.py:130): ground truth first
        return LpipsResult(out[:, 0], out[:, 1:])

    @torch.no_grad()
    def forward(self, pred, target, mask=None, normalize=False, spatial=False) -> torch.Tensor:
        """PerceptualLoss.forward (models/__init__.py:26-40): inputs in [-1, 1] (normalize=True: in [0, 1]) -> [B,1,1,1] fp32."""
        if mask is not None or spatial:
            raise NotImplementedError("LpipsAlex.forward: a mask and spatial=True are calls of their own: forward_masked, "
                                      "forward_spatial (and spatial, which dycheck's compute_lpips reduces)")
        a, b = _pair("LpipsAlex.forward", target, pred)
        out = self._run(a, b, UNIT_RANGE if normalize else 0)
        return out[:, 0].float().reshape(-1, 1, 1, 1)

    @torch.no_grad()
    def features(self, img) -> List[torch.Tensor]:
        """The five ReLU maps of img [B,3,H,W] in [0, 1] as [B,C,h,w] tensors (views of the kernel's channel-last storage)."""
        a, _ = _pair("LpipsAlex.features", img, img)
        B, _, H, W = a.shape
        taps = [torch.empty(2 * B, h, w, c, dtype=torch.float32, device=a.device)
                for (h, w), c in zip(tap_sizes(H, W), COUT)]
        self._run(a, a, UNIT_RANGE, taps=taps)
        return [t[0::2].permute(0, 3, 1, 2) for t in taps]
