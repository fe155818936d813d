"""Host-side handle on one dmad_engine (one per process per GPU).

PyTorch is plumbing here: device memory (torch tensors), the current HIP stream and
torch.distributed.  All arithmetic of the hot path runs inside libdmad_hip.so.

Order of this file: constants and the argument helpers; the weight loaders (fingerprint, fold functions); class Engine — construction,
weights, the pass walker and the shapers, then one section per part in the order of include/dmad.h (WaveNet, mel front-end, UNet,
spectrogram classifiers, the vote loops and their exact-vote mode, the query surfaces, NES / particle swarm, the baseline waveform
defenses, M5, Philox and measurement hooks); the standalone op hooks; bind_* / get_engine."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import warnings
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import DmadConfig, DmadError, check
from .synth import WRN_BLOCKS, WRN_WIDTHS  # noqa: F401  (WideResNet-28-10's geometry, stated once with the stand-in)
from .synth import DN_BLOCKS, DN_GROWTH, DN_LAYERS  # noqa: F401  (DenseNet-BC-100-12's, likewise)

BF16, FP32, EXACT = 0, 1, 2                       # enum dmad_precision
MODE_FAST, MODE_EXACT_VOTES, MODE_FP32 = 0, 1, 2  # enum dmad_mode (EXACT engines)
HALF_BF16, HALF_F16 = 0, 1                        # enum dmad_half_type: operand format of the 16-bit MFMA path
WAVE_16BIT, WAVE_FP32, WAVE_SPLIT = 0, 1, 2       # dmad_set_waveform_tier: WaveNet tier of the waveform-returning surfaces (EXACT engines)
NES_STREAM = 0x4E450000                           # DMAD_PHILOX_STREAM_NES: the Philox stream of the NES probe directions
PSO_STREAM = 0x50530000                           # DMAD_PHILOX_STREAM_PSO: + 0 positions, 1 velocities, 2 r1, 3 r2 of the particle swarm
# Recheck bound of the exact-vote mode: a Monte Carlo sample whose 16-bit-path top-2 logit margin is below it is
# re-evaluated on the higher tiers.  Let i be the exact path's arg-max and e = (16-bit logits) - (exact logits).  If the 16-bit
# margin is >= tau and the 16-bit leader were some j != i, then l~_j - l~_i >= tau with l_j - l_i <= 0, i.e. e_j - e_i >= tau:
# so the vote is unchanged whenever tau exceeds E = max_j |e_j - e_i|, the largest error of a logit DIFFERENCE AGAINST THE
# EXACT LEADER.  Measured on 9 x 4096 samples (3 clips x sigma 0.25 / 0.5 / 1.0, tools/gpu_flip_study.py,
# profiles/r02_flip_study.md): f16 operands E = 0.0244 (0.0287 over all pairs i, j; 35 flips, the largest at margin 0.011),
# bf16 operands 0.207 (0.221; 261 flips) -> bounds with ~1.4x headroom.  Overridable: DMAD_RECHECK_MARGIN / recheck_margin=.
DEFAULT_RECHECK_MARGIN = {1: 0.034, 0: 0.30}          # by dmad_half_type: HALF_F16, HALF_BF16
# The error a given eps error turns into is a property of the classifier.  With the calibrated synthetic ResNeXt29 (first pass of the
# exact-vote mode = f16 WaveNet + the classifier's split-f16 tier; tools/gpu_flip_study.py with CLASSIFIER=resnext29 FIRSTPASS=1,
# profiles/r05h_flip_study_resnext29_first_pass.json, 36 864 samples): E = 0.0303, Gaussian scale 0.0065 -> 1.5 x E = 0.045 = 7 scales,
# P(E >= 0.045) = 4.5e-11 per sample.  load_resnext29 widens the bound to this floor.
# (the bf16 entry is the f16 one scaled by the VGG table's ratio 0.30 / 0.034, NOT measured: calibrate before using bf16 operands with it)
DEFAULT_RECHECK_MARGIN_RESNEXT29 = {1: 0.045, 0: 0.40}
# The queued samples first go through the split-f16 tier (fp32 pipeline, three f16 MFMAs per product, ~22 significant bits);
# only those whose margin is inside ITS error bound reach the exact-fp32 path.
DEFAULT_RECHECK_MARGIN2 = 1e-3
# Spec-domain vote loop (BASELINE C5): the UNet's 16-bit tier runs the whole 26-evaluation chain on f16 operands; a sample whose
# top-2 logit margin is below this bound re-runs its chain on a higher tier.  Measured with tools/gpu_c5_flip_study.py at the bench's
# engine batch 2048 on the CALIBRATED synthetic VGG19_bn (profiles/r05c_c5_flip_study.json, 6 144 samples, sigma 0.5, t* 25): the same
# leader-difference statistic as DEFAULT_RECHECK_MARGIN, 0.084 max, Gaussian scale 0.0198 -> 0.13 = 1.5 x max = 6.6 scales:
# P(E >= 0.13) = 4.9e-10 per sample by the Gaussian tail (the pessimistic one here: the generalised-Pareto fit of the top 61 has a
# negative shape and ends below 0.10; profiles/r05c_c5_recheck_tail_fit.txt), 1.5e-12 with the margin condition.  Like every bound of
# this file it is a property of the WEIGHTS: calibrate (calibrate_spec_recheck / RobustCertificate(calibrate=...)) before certifying
# with real checkpoints — round 4's 0.5 belonged to an uncalibrated stand-in whose logits were 50 x larger.
DEFAULT_SPEC_RECHECK_MARGIN = 0.13
# ... and the samples it queues first re-run their chain on the UNet's split-f16 tier (fp32 pipeline, three f16 MFMAs per product); only
# those whose margin is inside THAT tier's error bound reach the exact-fp32 UNet (dmad_set_spec_recheck_margin2; < 0: no middle tier).
DEFAULT_SPEC_RECHECK_MARGIN2 = 5e-4          # 2.2 x the largest leader-difference error (2.3e-4) of the split-f16 chain on 6 144 samples (profiles/r05c_c5_flip_study.json)
# Tail rule shared by the committed default and calibrate_recheck (tools/fit_recheck_tail.py): with s the
# Gaussian scale of the per-sample leader-difference error, a bound of TAIL_Z * s keeps the modelled miss probability per
# sample (error beyond the bound AND an exact margin small enough to be overturned) at or below 1e-9.
TAIL_Z = 5.4
VGG19_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512, 'M']
# (H, C) of VGG19_bn's 16 post-ReLU conv maps on a 32 x 32 spectrogram: the conv slots of the VJP's tape (vgg_vjp_tape)
VGG_TAPE_MAPS = ((32, 64),) * 2 + ((16, 128),) * 2 + ((8, 256),) * 4 + ((4, 512),) * 4 + ((2, 512),) * 4
# WideResNet-28-10: (cin, cout, stride) of its 12 pre-activation blocks, and (H, C) of the 25 post-ReLU maps of the VJP's tape
# (wrn_vjp_tape): o = relu(bn1(x)) and h = relu(bn2(conv1(o))) of blocks 0..11, then the final map; 2 310 144 floats per spectrogram


def _wrn_tape_maps():
    maps, H = [], 32
    for cin, cout, stride in WRN_BLOCKS:
        maps += [(H, cin), (H // stride, cout)]
        H //= stride
    return tuple(maps) + ((8, 640),)


WRN_TAPE_MAPS = _wrn_tape_maps()
# DenseNet-BC-100-12: (H, C) of the 99 post-ReLU maps of dn_vjp_tape in forward order: o = relu(bn1(x)) and h of a block's 16 layers, then
# the transition's (or, behind dense3, the final) pre-activated map


def _dn_tape_maps():
    maps = []
    for H, c0, width in DN_BLOCKS:
        for i in range(DN_LAYERS):
            maps += [(H, c0 + DN_GROWTH * i), (H, 4 * DN_GROWTH)]
        maps.append((H, width))
    return tuple(maps)


DN_TAPE_MAPS = _dn_tape_maps()
KWS_BINS, KWS_CLASSES = 32, 4                      # mel bins and classes of the attention-CRNN keyword spotter (csrc/kws.h)
KWS_MAX_T = 644                                    # kKwsMaxT: the longest row dmad_kws_* serve (40 GRU steps)
M5_CHANNELS = (32, 32, 64, 64)                     # output channels of M5's four conv blocks (n_channel = 32)
# the WaveNet geometry an engine is created with unless the caller names another one
DEFAULT_WAVENET = dict(res_channels=256, skip_channels=256, num_res_layers=36, dilation_cycle=12,
                       diffusion_step_embed_dim_in=128, diffusion_step_embed_dim_mid=512, diffusion_step_embed_dim_out=512)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _as_np(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().float().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _f32(t):
    return None if t is None else t.detach().contiguous().float()


def _f64(v) -> np.ndarray:
    """a state dict entry in float64 on the host: what the fold functions compute in"""
    return v.detach().cpu().double().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64)


def _on_gpu(*tensors):
    if not all(t.is_cuda for t in tensors):
        raise DmadError('input must live on the GPU (the dmad engine has no CPU path)')


def _floats(n: int, *seqs):
    """host coefficient sequences -> one (C.c_float * n) each"""
    return [(C.c_float * n)(*[float(v) for v in a]) for a in seqs]


# What Engine._passes evaluates once per pass, as a(s, e) for the rows [s, e) of the batch:
def _per(t: Optional[torch.Tensor], k: int = 1):
    """a per-row tensor (contiguous): the pointer to its rows [k * s, k * e) (k rows per clip: the VP-SDE trajectory); None stays None"""
    if t is None:
        return None
    base, step = t.data_ptr(), k * t.stride(0) * t.element_size()
    return lambda s, e: C.c_void_p(base + s * step)


def _cols(z: Optional[torch.Tensor]):
    """the explicit noise [S + 1, B, W] of a VP-SDE chain: the pointer to z[:, s:e] as a fresh contiguous copy per pass, which lives
    until the next pass replaces it; None stays None"""
    if z is None:
        return None
    held = []

    def cut(s, e):
        held[:] = [z[:, s:e].contiguous()]
        return _ptr(held[0])
    return cut


def _N(s, e):
    """the row count of the pass"""
    return e - s


def _key(sample0):
    """the Philox key offset of the pass's first row"""
    sample0 = int(sample0)
    return lambda s, e: sample0 + s


# ---------------------------------------------------------------------- weights: fingerprint and the fold functions
def state_fingerprint(sd: Dict[str, object]) -> str:
    """Content hash of a state dict (names, shapes, bytes; BatchNorm's num_batches_tracked counters excepted: they do not
    enter inference): identifies WHICH weights an engine holds."""
    h = hashlib.sha1()
    for k in sorted(sd):
        if k.endswith('num_batches_tracked'):
            continue
        v = sd[k]
        a = v.detach().cpu().contiguous().numpy() if isinstance(v, torch.Tensor) else np.ascontiguousarray(v)
        h.update(k.encode()); h.update(str(a.dtype).encode()); h.update(str(a.shape).encode())
        h.update(memoryview(a.reshape(-1)).cast('B'))
    return h.hexdigest()


def fold_wavenet_state_dict(sd: Dict[str, object], num_res_layers: int) -> Dict[str, np.ndarray]:
    """Reference checkpoint layout -> folded fp32 arrays named as in dmad.h.
    Weight norm is folded with torch._weight_norm, the very op nn.utils.weight_norm evaluates on each
    forward of the reference (WaveNet.py:27-28,66-72)."""
    def T(k):
        v = sd[k]
        return v.detach().cpu().float() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v, dtype=np.float32))

    def fold(prefix):
        return torch._weight_norm(T(prefix + '.weight_v'), T(prefix + '.weight_g'), 0)

    out = {'init.w': fold('init_conv.0.conv').reshape(256), 'init.b': T('init_conv.0.conv.bias'),
           'fc_t1.w': T('residual_layer.fc_t1.weight'), 'fc_t1.b': T('residual_layer.fc_t1.bias'),
           'fc_t2.w': T('residual_layer.fc_t2.weight'), 'fc_t2.b': T('residual_layer.fc_t2.bias')}
    for n in range(num_res_layers):
        p = 'residual_layer.residual_blocks.%d' % n
        out['fc_t.%d.w' % n] = T(p + '.fc_t.weight'); out['fc_t.%d.b' % n] = T(p + '.fc_t.bias')
        out['dil.%d.w' % n] = fold(p + '.dilated_conv_layer.conv'); out['dil.%d.b' % n] = T(p + '.dilated_conv_layer.conv.bias')
        out['res.%d.w' % n] = fold(p + '.res_conv').reshape(256, 256); out['res.%d.b' % n] = T(p + '.res_conv.bias')
        out['skip.%d.w' % n] = fold(p + '.skip_conv').reshape(256, 256); out['skip.%d.b' % n] = T(p + '.skip_conv.bias')
    out['f0.w'] = fold('final_conv.0.conv').reshape(256, 256); out['f0.b'] = T('final_conv.0.conv.bias')
    out['f2.w'] = T('final_conv.2.conv.weight').reshape(256); out['f2.b'] = T('final_conv.2.conv.bias').reshape(1)
    return {k: _as_np(v) for k, v in out.items()}


def _fold_bn(sd, bn: str, eps: float, conv_bias: Optional[str] = None):
    """eval-mode BatchNorm `bn` behind a conv -> (scale, shift) in float64: scale = gamma / sqrt(var + eps),
    shift = (bias - mean) * scale + beta (a conv without bias: -mean * scale + beta, the same bits as beta - mean * scale)."""
    scale = _f64(sd[bn + '.weight']) / np.sqrt(_f64(sd[bn + '.running_var']) + eps)
    mean = _f64(sd[bn + '.running_mean'])
    return scale, (-mean if conv_bias is None else _f64(sd[conv_bias]) - mean) * scale + _f64(sd[bn + '.bias'])


def fold_vgg19_bn_state_dict(sd: Dict[str, object], eps: float = 1e-5) -> Dict[str, np.ndarray]:
    """models/vgg.py vgg19_bn state dict -> conv weights + eval-mode BatchNorm folded to scale/shift
    (float64 on the host, rounded once):  y = scale * conv(x) + shift,
    scale = gamma / sqrt(var + eps), shift = (bias - mean) * scale + beta."""
    out, idx, li = {}, 0, 0
    for v in VGG19_CFG:
        if v == 'M':
            idx += 1
            continue
        out['vgg.conv%d.w' % li] = _f64(sd['features.%d.weight' % idx])
        out['vgg.conv%d.scale' % li], out['vgg.conv%d.shift' % li] = _fold_bn(sd, 'features.%d' % (idx + 1), eps, 'features.%d.bias' % idx)
        idx += 3
        li += 1
    for j, i in enumerate((0, 3, 6)):
        out['vgg.fc%d.w' % j] = _f64(sd['classifier.%d.weight' % i])
        out['vgg.fc%d.b' % j] = _f64(sd['classifier.%d.bias' % i])
    return {k: _as_np(v) for k, v in out.items()}


def fold_resnext29_state_dict(sd: Dict[str, object], eps: float = 1e-5) -> Dict[str, np.ndarray]:
    """models/resnext.py CifarResNeXt (8x64d, depth 29) state dict -> conv weights + eval-mode BatchNorm folded to
    scale/shift per conv (float64 on the host, rounded once); bottleneck i = 3 * (stage - 1) + k."""
    out = {'rx.conv1.w': _f64(sd['conv_1_3x3.weight'])}
    out['rx.conv1.scale'], out['rx.conv1.shift'] = _fold_bn(sd, 'bn_1', eps)
    for st in (1, 2, 3):
        for k in range(3):
            src = 'stage_%d.stage_%d_bottleneck_%d.' % (st, st, k)
            dst = 'rx.b%d.' % (3 * (st - 1) + k)
            for conv, norm, name in (('conv_reduce', 'bn_reduce', 'reduce'), ('conv_conv', 'bn', 'conv'), ('conv_expand', 'bn_expand', 'expand')):
                w = _f64(sd[src + conv + '.weight'])
                out[dst + name + '.w'] = w.reshape(w.shape[0], w.shape[1]) if name != 'conv' else w
                out[dst + name + '.scale'], out[dst + name + '.shift'] = _fold_bn(sd, src + norm, eps)
            if src + 'shortcut.shortcut_conv.weight' in sd:
                w = _f64(sd[src + 'shortcut.shortcut_conv.weight'])
                out[dst + 'short.w'] = w.reshape(w.shape[0], w.shape[1])
                out[dst + 'short.scale'], out[dst + 'short.shift'] = _fold_bn(sd, src + 'shortcut.shortcut_bn', eps)
    out['rx.fc.w'] = _f64(sd['classifier.weight'])
    out['rx.fc.b'] = _f64(sd['classifier.bias'])
    return {k: _as_np(v) for k, v in out.items()}


def fold_wideresnet_state_dict(sd: Dict[str, object], eps: float = 1e-5, dtype=np.float32) -> Dict[str, np.ndarray]:
    """models/wideresnet.py WideResNet(depth=28, widen_factor=10, in_channels=1) state dict -> the `wrn.*` arrays of include/dmad.h: each
    block's bn1 (the pre-activation on the residual stream), bn2 (conv1's epilogue) and the final bn folded to scale / shift in float64
    and rounded once; shortcut weights as [cout, cin]; block i = 4 * stage + k.  Any other geometry is refused (DmadError).  dtype: what the float64 folds are
    rounded to (np.float64: the arrays before the rounding, for the tests)."""
    def shape(k):
        return tuple(int(d) for d in sd[k].shape) if k in sd else None

    if shape('conv1.weight') != (16, 1, 3, 3):
        raise DmadError('only WideResNet-28-10 with 1 input channel is built natively: conv1.weight is %s, not (16, 1, 3, 3)' % (shape('conv1.weight'),))
    if shape('fc.weight') is None or shape('fc.weight')[1:] != (640,) or 'block1.layer.4.conv1.weight' in sd or 'block1.layer.3.conv1.weight' not in sd:
        raise DmadError('only WideResNet-28-10 is built natively: four blocks per stage and a 640-wide head (fc.weight is %s)' % (shape('fc.weight'),))
    out = {'wrn.conv1.w': _f64(sd['conv1.weight'])}
    for i, (cin, cout, _) in enumerate(WRN_BLOCKS):
        src, dst = 'block%d.layer.%d.' % (i // 4 + 1, i % 4), 'wrn.b%d.' % i
        if shape(src + 'conv1.weight') != (cout, cin, 3, 3) or shape(src + 'conv2.weight') != (cout, cout, 3, 3):
            raise DmadError('only WideResNet-28-10 is built natively: %sconv1.weight is %s, not %s' % (src, shape(src + 'conv1.weight'), (cout, cin, 3, 3)))
        out[dst + 'bn1.scale'], out[dst + 'bn1.shift'] = _fold_bn(sd, src + 'bn1', eps)
        out[dst + 'conv1.w'] = _f64(sd[src + 'conv1.weight'])
        out[dst + 'conv1.scale'], out[dst + 'conv1.shift'] = _fold_bn(sd, src + 'bn2', eps)
        out[dst + 'conv2.w'] = _f64(sd[src + 'conv2.weight'])
        if cin != cout:
            out[dst + 'short.w'] = _f64(sd[src + 'convShortcut.weight']).reshape(cout, cin)
    out['wrn.bn.scale'], out['wrn.bn.shift'] = _fold_bn(sd, 'bn1', eps)
    out['wrn.fc.w'] = _f64(sd['fc.weight'])
    out['wrn.fc.b'] = _f64(sd['fc.bias'])
    return {k: np.ascontiguousarray(v, dtype=dtype) for k, v in out.items()}


def kws_steps(T: int) -> int:
    """GRU steps of a T-frame spectrogram: Conv1d(k=5, stride 2) then Conv1d(k=1, stride 8)"""
    return ((T - 5) // 2) // 8 + 1 if T >= 5 else 0


def kws_frames(L: int) -> int:
    """spectrogram frames of an L-sample clip behind the KWS mel front-end (hop 200, center=True)"""
    return 1 + int(L) // 200


def fold_densenet_state_dict(sd: Dict[str, object], eps: float = 1e-5, dtype=np.float32) -> Dict[str, np.ndarray]:
    """models/densenet.py DenseNet(depth=100, growthRate=12, compressionRate=2, in_channels=1) state dict -> the `dn.*` arrays of
    include/dmad.h: every BatchNorm folded to scale / shift in float64 and rounded once (_fold_bn); the 1x1 weights as [cout, cin]; layer
    l = 16 * block + i.  Any other geometry is refused (DmadError).  dtype: what the float64 folds are rounded to (np.float64: the arrays
    before the rounding, for the tests)."""
    def shape(k):
        return tuple(int(d) for d in sd[k].shape) if k in sd else None

    if shape('conv1.weight') != (2 * DN_GROWTH, 1, 3, 3):
        raise DmadError('only DenseNet-BC-100-12 with 1 input channel is built natively: conv1.weight is %s, not (24, 1, 3, 3)' % (shape('conv1.weight'),))
    if shape('fc.weight') is None or shape('fc.weight')[1:] != (DN_BLOCKS[2][2],) or 'dense1.16.conv1.weight' in sd or 'dense1.15.conv2.weight' not in sd:
        raise DmadError('only DenseNet-BC-100-12 is built natively: 16 bottleneck layers per block and a 342-wide head (fc.weight is %s)' % (shape('fc.weight'),))
    out = {'dn.conv1.w': _f64(sd['conv1.weight'])}
    for blk, (_, c0, width) in enumerate(DN_BLOCKS):
        for i in range(DN_LAYERS):
            src, dst, cin = 'dense%d.%d.' % (blk + 1, i), 'dn.l%d.' % (DN_LAYERS * blk + i), c0 + DN_GROWTH * i
            if shape(src + 'conv1.weight') != (4 * DN_GROWTH, cin, 1, 1) or shape(src + 'conv2.weight') != (DN_GROWTH, 4 * DN_GROWTH, 3, 3):
                raise DmadError('only DenseNet-BC-100-12 is built natively: %sconv1.weight is %s, not %s' % (src, shape(src + 'conv1.weight'), (48, cin, 1, 1)))
            out[dst + 'bn1.scale'], out[dst + 'bn1.shift'] = _fold_bn(sd, src + 'bn1', eps)
            out[dst + 'conv1.w'] = _f64(sd[src + 'conv1.weight']).reshape(4 * DN_GROWTH, cin)
            out[dst + 'conv1.scale'], out[dst + 'conv1.shift'] = _fold_bn(sd, src + 'bn2', eps)
            out[dst + 'conv2.w'] = _f64(sd[src + 'conv2.weight'])
        if blk < 2:
            src, dst, cout = 'trans%d.' % (blk + 1), 'dn.t%d.' % blk, DN_BLOCKS[blk + 1][1]
            if shape(src + 'conv1.weight') != (cout, width, 1, 1):
                raise DmadError('only DenseNet-BC-100-12 is built natively: %sconv1.weight is %s, not %s' % (src, shape(src + 'conv1.weight'), (cout, width, 1, 1)))
            out[dst + 'bn.scale'], out[dst + 'bn.shift'] = _fold_bn(sd, src + 'bn1', eps)
            out[dst + 'conv.w'] = _f64(sd[src + 'conv1.weight']).reshape(cout, width)
    out['dn.bn.scale'], out['dn.bn.shift'] = _fold_bn(sd, 'bn', eps)
    out['dn.fc.w'] = _f64(sd['fc.weight'])
    out['dn.fc.b'] = _f64(sd['fc.bias'])
    return {k: np.ascontiguousarray(v, dtype=dtype) for k, v in out.items()}


def fold_m5_state_dict(sd: Dict[str, object], stride: int = 16, eps: float = 1e-5) -> Dict[str, np.ndarray]:
    """M5Net.M5 state dict -> the `m5.*` arrays of include/dmad.h: the conv weights as they are, each eval-BatchNorm folded (in float64)
    into s = gamma / sqrt(var + eps) and shift = beta + (bias - mean) * s, fc1, and conv1's stride (the one geometry field no tensor
    shape shows).  The geometry is checked by dmad_finalize_weights (DMAD_ERR_SHAPE)."""
    out = {'m5.stride': np.array([float(stride)], dtype=np.float32)}
    for i in (1, 2, 3, 4):
        out['m5.conv%d.w' % i] = _f64(sd['conv%d.weight' % i])
        out['m5.scale%d' % i], out['m5.shift%d' % i] = _fold_bn(sd, 'bn%d' % i, eps, 'conv%d.bias' % i)
    out['m5.fc.w'] = _f64(sd['fc1.weight'])
    out['m5.fc.b'] = _f64(sd['fc1.bias'])
    return {k: _as_np(v) for k, v in out.items()}


class Engine:
    """One libdmad_hip engine bound to the current CUDA(HIP) device."""

    @staticmethod
    def geometry(wavenet_config: Optional[dict]) -> tuple:
        wc = dict(DEFAULT_WAVENET)
        wc.update({k: v for k, v in (wavenet_config or {}).items() if k in wc})
        return tuple(sorted(wc.items()))

    def __init__(self, wavenet_config: Optional[dict] = None, clip_len: int = 16000, max_batch: int = 64,
                 num_classes: int = 10, precision: int = BF16, with_classifier: bool = True, recheck_batch: int = 0,
                 recheck_margin: Optional[float] = None, half_type: Optional[int] = None, with_wavenet: bool = True):
        if not torch.cuda.is_available():
            raise DmadError('no MI355X/HIP device visible: the dmad engine has no CPU path')
        self.lib = _lib.load()
        wc = dict(DEFAULT_WAVENET)
        wc.update(wavenet_config or {})
        if wc.get('in_channels', 1) != 1 or wc.get('out_channels', 1) != 1:
            raise DmadError('only in_channels = out_channels = 1 is supported')
        if half_type is None:    # f16 operands for the exact-vote engine (smaller recheck band), bf16 for the plain 16-bit engine
            half_type = {'bf16': HALF_BF16, 'f16': HALF_F16}[os.environ.get('DMAD_HALF_TYPE', 'f16' if precision == EXACT else 'bf16').lower()]
        self.cfg = DmadConfig(wc['res_channels'], wc['skip_channels'], wc['num_res_layers'], wc['dilation_cycle'],
                              wc['diffusion_step_embed_dim_in'], wc['diffusion_step_embed_dim_mid'],
                              wc['diffusion_step_embed_dim_out'], clip_len, max_batch, num_classes, precision,
                              1 if with_classifier else 0, recheck_batch, half_type, 1 if with_wavenet else 0)
        self.half_type = half_type
        self.with_wavenet = bool(with_wavenet)
        self.L, self.max_batch, self.num_classes, self.precision = clip_len, max_batch, num_classes, precision
        self.num_res_layers = wc['num_res_layers']
        self.wavenet_geometry = Engine.geometry(wc)
        self.device = torch.device('cuda', torch.cuda.current_device())
        h = C.c_void_p()
        check(self.lib.dmad_create(C.byref(self.cfg), C.byref(h)))
        self._h = h
        self.has_wavenet = False
        self.has_classifier = False
        self.has_unet = False
        self.has_m5 = False
        self.m5_owner, self.m5_classes, self.m5_maps = None, 0, ()
        self.has_kws, self.kws_owner = False, None
        self.vjp_batch = self.unet_vjp_batch = self.classifier_vjp_batch = self.vgg_vjp_batch = self.wrn_vjp_batch = self.dn_vjp_batch = 0     # rows per pass the VJP workspaces are reserved for
        # which weights are resident (state_fingerprint): a module that binds to an engine holding OTHER weights must
        # not silently run them
        self.wavenet_owner = self.classifier_owner = self.unet_owner = None
        self.classifier_kind = None
        self.mode = {BF16: MODE_FAST, FP32: MODE_FP32, EXACT: MODE_EXACT_VOTES}[precision]
        self.calibration = None                # what the last calibrate_recheck() observed
        self.waveform_tier = WAVE_SPLIT if precision == EXACT else WAVE_16BIT
        # what calibrations may never go below: the committed defaults, or a wider bound the caller chose (constructor / environment /
        # a direct set_recheck_margin call)
        self.floor1, self.floor2, self.floor_spec = DEFAULT_RECHECK_MARGIN[half_type], DEFAULT_RECHECK_MARGIN2, DEFAULT_SPEC_RECHECK_MARGIN
        self.floor_spec2 = DEFAULT_SPEC_RECHECK_MARGIN2
        self.spec_calibration = None
        if precision == EXACT:
            wt = os.environ.get('DMAD_WAVEFORM_TIER')
            if wt:
                self.set_waveform_tier({'16bit': WAVE_16BIT, 'fp32': WAVE_FP32, 'split': WAVE_SPLIT}[wt.lower()])
            if recheck_margin is None:
                recheck_margin = float(os.environ.get('DMAD_RECHECK_MARGIN', DEFAULT_RECHECK_MARGIN[half_type]))
            self.set_recheck_margin(recheck_margin)
            self.set_recheck_margin2(float(os.environ.get('DMAD_RECHECK_MARGIN2', DEFAULT_RECHECK_MARGIN2)))
            self.set_spec_recheck_margin(float(os.environ.get('DMAD_SPEC_RECHECK_MARGIN', DEFAULT_SPEC_RECHECK_MARGIN)))
            self.set_spec_recheck_margin2(float(os.environ.get('DMAD_SPEC_RECHECK_MARGIN2', DEFAULT_SPEC_RECHECK_MARGIN2)))

    def close(self):
        if getattr(self, '_h', None):
            torch.cuda.synchronize()
            self.lib.dmad_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def _load(self, arrays: Dict[str, np.ndarray]):
        for name, a in arrays.items():
            a = np.ascontiguousarray(a, dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            check(self.lib.dmad_load_weight(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))
        check(self.lib.dmad_finalize_weights(self._h))
        note = self.lib.dmad_last_warning()
        if note:
            warnings.warn('dmad engine: ' + note.decode(), RuntimeWarning, stacklevel=3)

    def load_wavenet(self, state_dict):
        if self.has_wavenet:
            raise DmadError('WaveNet weights are already loaded into this engine')
        self._load(fold_wavenet_state_dict(state_dict, self.num_res_layers))
        self.has_wavenet = True
        self.wavenet_owner = state_fingerprint(state_dict)

    def load_unet(self, state_dict):
        """improved_diffusion.unet.UNetModel state dict (synth.UNET_CONFIG geometry) -> engine, names prefixed 'un.'."""
        if self.has_unet:
            raise DmadError('UNet weights are already loaded into this engine')
        self._load({'un.' + k: _as_np(_f64(v)) for k, v in state_dict.items()})
        self.has_unet = True
        self.unet_owner = state_fingerprint(state_dict)

    def load_vgg19_bn(self, state_dict):
        if self.has_classifier:
            raise DmadError('classifier weights are already loaded into this engine')
        self._load(fold_vgg19_bn_state_dict(state_dict))
        self.has_classifier = True
        self.classifier_owner, self.classifier_kind = state_fingerprint(state_dict), 'vgg19_bn'

    def load_resnext29(self, state_dict):
        if self.has_classifier:
            raise DmadError('classifier weights are already loaded into this engine')
        self._load(fold_resnext29_state_dict(state_dict))
        self.has_classifier = True
        self.classifier_owner, self.classifier_kind = state_fingerprint(state_dict), 'resnext29'
        if self.precision == EXACT:            # the committed bound for this classifier kind (widen-only, like a calibration)
            self.floor1 = max(self.floor1, self._committed_margin1())
            if self.recheck_margin < self.floor1:
                self.set_recheck_margin(self.floor1, calibrated=True)

    def load_wideresnet28_10(self, state_dict):
        """models/wideresnet.py WideResNet-28-10 state dict -> engine (names prefixed 'wrn.').  No recheck bound has been measured for this
        classifier: on an EXACT engine the vote loops refuse it in the exact-vote mode (DmadError with the library's reason)."""
        if self.has_classifier:
            raise DmadError('classifier weights are already loaded into this engine')
        self._load(fold_wideresnet_state_dict(state_dict))
        self.has_classifier = True
        self.classifier_owner, self.classifier_kind = state_fingerprint(state_dict), 'wideresnet28_10'

    def load_densenet_bc_100_12(self, state_dict):
        """models/densenet.py DenseNet-BC-100-12 state dict -> engine (names prefixed 'dn.').  No recheck bound has been measured for this
        classifier: on an EXACT engine the vote loops refuse it in the exact-vote mode (DmadError with the library's reason)."""
        if self.has_classifier:
            raise DmadError('classifier weights are already loaded into this engine')
        self._load(fold_densenet_state_dict(state_dict))
        self.has_classifier = True
        self.classifier_owner, self.classifier_kind = state_fingerprint(state_dict), 'densenet_bc_100_12'

    def load_m5(self, state_dict, stride: int = 16):
        """M5Net.M5 state dict -> engine (names prefixed 'm5.'); a part of its own beside the spectrogram classifier.  stride: conv1's."""
        if self.has_m5:
            raise DmadError('M5 weights are already loaded into this engine')
        arrays = fold_m5_state_dict(state_dict, stride)
        self._load(arrays)
        self.has_m5 = True
        self.m5_owner, self.m5_classes = state_fingerprint(state_dict), int(arrays['m5.fc.w'].shape[0])
        t, maps = (self.L - arrays['m5.conv1.w'].shape[2]) // 16 + 1, []
        for c in M5_CHANNELS:                 # (channels, pooled frames) of the four blocks: the shapes of m5_tape
            maps.append((c, t // 4))
            t = t // 4 - 2
        self.m5_maps = tuple(maps)

    def load_kws(self, state_dict, kernel_size=(20, 5), stride=(8, 2)):
        """RCNN_KWS.model.KWSModel state dict -> engine (its 24 tensors under 'kws.' + key, and the constructor's kernel_size / stride,
        which no tensor shows); a part of its own beside the spectrogram classifier and M5."""
        if self.has_kws:
            raise DmadError('KWS weights are already loaded into this engine')
        arrays = {'kws.' + k: _as_np(v) for k, v in state_dict.items()}
        arrays['kws.kernel_size'] = np.array(kernel_size, dtype=np.float32)
        arrays['kws.stride'] = np.array(stride, dtype=np.float32)
        self._load(arrays)
        self.has_kws = True
        self.kws_owner = state_fingerprint(state_dict)

    def bind(self, part: str, state_dict, loader) -> None:
        """Make `state_dict` the resident weights of `part` ('wavenet' / 'classifier' / 'unet' / 'm5' / 'kws'): upload them if the
        part is empty, accept them if they ARE the resident ones, refuse anything else (an engine holds one weight set per
        part for its lifetime; use get_engine(fresh=True) / Engine(...) for a second model)."""
        owner = getattr(self, part + '_owner')
        if not getattr(self, 'has_' + part):
            loader(state_dict)
            return
        fp = state_fingerprint(state_dict)
        if owner != fp:
            raise DmadError('this engine already holds different %s weights (resident %s..., offered %s...): bind the module to '
                            'its own engine (dmad_hip.engine.get_engine(fresh=True))' % (part, str(owner)[:10], fp[:10]))

    # ------------------------------------------------------------------ the pass walker, the shapers, the output builders
    def _passes(self, fn, B: int, *args):
        """Run the export `fn` on B rows in passes of max_batch: the one place where a batch is cut.  args: the export's arguments
        between the handle and the stream, in its order.  A callable among them is evaluated once per pass as a(s, e) for the rows
        [s, e) (_per, _cols, _N, _key above) and its value goes in; everything else, None included, is passed as it is."""
        call = [self._h, *args, _stream()]
        live = [(i, a) for i, a in enumerate(call) if callable(a)]
        for s in range(0, B, self.max_batch):
            e = min(B, s + self.max_batch)
            for i, a in live:
                call[i] = a(s, e)
            check(fn(*call))

    def _mapped(self, fn, x: torch.Tensor, *mid) -> torch.Tensor:
        """the exports that take the rows first and write an output of their shape last: walk `fn` over x, -> that output"""
        out = torch.empty_like(x)
        self._passes(fn, x.shape[0], _per(x), *mid, _per(out))
        return out

    def _wave(self, x: torch.Tensor) -> torch.Tensor:
        _on_gpu(x)
        x = x.detach()
        if x.dim() == 3:
            assert x.shape[1] == 1, 'expected [B,1,L]'
            x = x[:, 0]
        assert x.dim() == 2 and x.shape[1] == self.L, 'expected [B,%d], got %s' % (self.L, tuple(x.shape))
        return x.contiguous().float()

    def _spec(self, x: torch.Tensor) -> torch.Tensor:
        _on_gpu(x)
        x = x.detach()
        if x.dim() == 4:
            assert x.shape[1] == 1, 'expected [B,1,32,32]'
            x = x[:, 0]
        assert x.dim() == 3 and tuple(x.shape[1:]) == (32, 32), 'expected [B,32,32], got %s' % (tuple(x.shape),)
        return x.contiguous().float()

    @staticmethod
    def _rows(x: torch.Tensor, width: int, name: str = 'x') -> torch.Tensor:
        _on_gpu(x)
        x = x.detach()
        if x.dim() != 2 or x.shape[1] != width:
            raise DmadError('%s must be [B, %d], not %s' % (name, width, tuple(x.shape)))
        return x.contiguous().float()

    def _clip(self, clip: torch.Tensor) -> torch.Tensor:
        """the one clip of a vote loop / eval_samples call"""
        clip = clip.detach().reshape(-1).contiguous().float()
        assert clip.is_cuda and clip.numel() == self.L
        return clip

    @staticmethod
    def _logits_pair(rows: int, width: int, device):
        """(logits [rows, width] float32, decisions int32 [rows]) of the query surfaces"""
        return torch.empty((rows, width), device=device, dtype=torch.float32), torch.empty((rows,), device=device, dtype=torch.int32)

    def _reserve(self, name: str, max_batch: int, recorded: Optional[int] = None):
        """dmad_reserve_<name>: the four VJP workspaces; <name>_batch keeps the largest reservation made"""
        check(getattr(self.lib, 'dmad_reserve_' + name)(self._h, int(max_batch)))
        setattr(self, name + '_batch', max(getattr(self, name + '_batch'), int(max_batch) if recorded is None else recorded))

    # ------------------------------------------------------------------ WaveNet (the DiffWave purifiers)
    def wavenet_eps(self, x_t: torch.Tensor, t: int) -> torch.Tensor:
        return self._mapped(self.lib.dmad_wavenet_eps, self._wave(x_t), int(t), _N)

    def wavenet_eps_path(self, x_t: torch.Tensor, t: int, path: int) -> torch.Tensor:
        """eps-network on an explicit path of an EXACT engine: 0 mode default, 1 exact fp32, 2 split-f16 (three MFMAs per product)."""
        return self._mapped(self.lib.dmad_wavenet_eps_path, self._wave(x_t), int(t), _N, int(path))

    def one_shot(self, x_t: torch.Tensor, t: int, c_a: float, c_b: float) -> torch.Tensor:
        return self._mapped(self.lib.dmad_one_shot, self._wave(x_t), int(t), float(c_a), float(c_b), _N)

    def ddpm_step(self, x: torch.Tensor, t: int, c_eps: float, c_div: float, c_sig: float, z: Optional[torch.Tensor],
                  seed: int = 0, sample0: int = 0):
        """in place on x ([B, L] contiguous fp32 CUDA)."""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32
        zz = None if z is None else self._wave(z)
        self._passes(self.lib.dmad_ddpm_step, x.shape[0], _per(x), int(t), float(c_eps), float(c_div), float(c_sig), _per(zz), int(seed),
                     _key(sample0), _N)
        return x

    def diffuse(self, x0: torch.Tensor, c_a: float, c_b: float, z: Optional[torch.Tensor], seed: int = 0, sample0: int = 0):
        x = self._wave(x0)
        zz = None if z is None else self._wave(z)
        return self._mapped(self.lib.dmad_diffuse, x, float(c_a), float(c_b), _per(zz), int(seed), _key(sample0), _N)

    def ddpm_purify(self, x0: torch.Tensor, t_star: int, c_a: float, c_b: float, c_eps, c_div, c_sig, seed: int = 0, sample0: int = 0):
        """DiffWave.forward with device noise in one library call per chunk; c_eps / c_div / c_sig: t_star floats each."""
        return self._mapped(self.lib.dmad_ddpm_purify, self._wave(x0), int(t_star), float(c_a), float(c_b), *_floats(t_star, c_eps, c_div, c_sig),
                            int(seed), _key(sample0), _N)

    def reserve_vjp(self, max_batch: int):
        """dmad_reserve_vjp: the workspace of wavenet_eps_vjp for up to max_batch clips per pass (capped at the engine's fp32 pass
        size; a larger reservation replaces a smaller one).  FP32 / EXACT engines; DmadError otherwise."""
        self._reserve('vjp', max_batch)

    def _eps_vjp(self, fn, shaper, x_t, t, g_eps, want_eps):
        """wavenet_eps_vjp / unet_eps_vjp: the export `fn` on maps that `shaper` (_wave / _spec) checks"""
        x, g = shaper(x_t), shaper(g_eps)
        if g.shape != x.shape:
            raise DmadError('g_eps has shape %s, x_t %s' % (tuple(g.shape), tuple(x.shape)))
        gx = torch.empty_like(x)
        eps = torch.empty_like(x) if want_eps else None
        self._passes(fn, x.shape[0], _per(x), int(t), _N, _per(g), _per(gx), _per(eps))
        return (gx, eps) if want_eps else gx

    def wavenet_eps_vjp(self, x_t: torch.Tensor, t: int, g_eps: torch.Tensor, want_eps: bool = False):
        """g_x = (d eps / d x_t)^T g_eps for eps = WaveNet((x_t, t * ones)) on the exact-fp32 path ([B,L] or [B,1,L] -> [B,L]).
        want_eps: also return eps, bit-identical to wavenet_eps_path(x_t, t, 1).  Needs reserve_vjp first (DmadError otherwise)."""
        return self._eps_vjp(self.lib.dmad_wavenet_eps_vjp, self._wave, x_t, t, g_eps, want_eps)

    # ------------------------------------------------------------------ clips of any length on the exact-fp32 path (dmad_*_len)
    @staticmethod
    def _wave_len(x: torch.Tensor, like: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[B, len] or [B, 1, len] -> contiguous fp32 [B, len]; the length is the tensor's (the library checks 1 <= len <= clip_len)"""
        _on_gpu(x)
        x = x.detach()
        if x.dim() == 3:
            assert x.shape[1] == 1, 'expected [B,1,len]'
            x = x[:, 0]
        assert x.dim() == 2, 'expected [B,len], got %s' % (tuple(x.shape),)
        if like is not None and x.shape != like.shape:
            raise DmadError('shape %s does not match the waveforms %s' % (tuple(x.shape), tuple(like.shape)))
        return x.contiguous().float()

    def wavenet_eps_len(self, x_t: torch.Tensor, t: int) -> torch.Tensor:
        """dmad_wavenet_eps_len: eps on the exact-fp32 path for clips of x_t's own length, 1 <= len <= clip_len.  At len == clip_len
        the bits of wavenet_eps_path(x_t, t, 1)."""
        x = self._wave_len(x_t)
        return self._mapped(self.lib.dmad_wavenet_eps_len, x, int(t), _N, x.shape[1])

    def wavenet_eps_vjp_len(self, x_t: torch.Tensor, t: int, g_eps: torch.Tensor, want_eps: bool = False):
        """dmad_wavenet_eps_vjp_len: wavenet_eps_vjp for clips of x_t's own length (the same reserve_vjp reservation)."""
        x = self._wave_len(x_t)
        g = self._wave_len(g_eps, x)
        gx = torch.empty_like(x)
        eps = torch.empty_like(x) if want_eps else None
        self._passes(self.lib.dmad_wavenet_eps_vjp_len, x.shape[0], _per(x), int(t), _N, x.shape[1], _per(g), _per(gx), _per(eps))
        return (gx, eps) if want_eps else gx

    def diffuse_len(self, x0: torch.Tensor, c_a: float, c_b: float, z: Optional[torch.Tensor], seed: int = 0, sample0: int = 0):
        x = self._wave_len(x0)
        zz = None if z is None else self._wave_len(z, x)
        return self._mapped(self.lib.dmad_diffuse_len, x, float(c_a), float(c_b), _per(zz), int(seed), _key(sample0), _N, x.shape[1])

    def ddpm_step_len(self, x: torch.Tensor, t: int, c_eps: float, c_div: float, c_sig: float, z: Optional[torch.Tensor],
                      seed: int = 0, sample0: int = 0):
        """in place on x ([B, len] contiguous fp32 CUDA)."""
        assert x.is_cuda and x.dim() == 2 and x.is_contiguous() and x.dtype == torch.float32
        zz = None if z is None else self._wave_len(z, x)
        self._passes(self.lib.dmad_ddpm_step_len, x.shape[0], _per(x), int(t), float(c_eps), float(c_div), float(c_sig), _per(zz), int(seed),
                     _key(sample0), _N, x.shape[1])
        return x

    def ddpm_purify_len(self, x0: torch.Tensor, t_star: int, c_a: float, c_b: float, c_eps, c_div, c_sig, seed: int = 0, sample0: int = 0):
        """ddpm_purify for clips of x0's own length: the draws are the first len values of the fixed-length call's."""
        x = self._wave_len(x0)
        return self._mapped(self.lib.dmad_ddpm_purify_len, x, int(t_star), float(c_a), float(c_b), *_floats(t_star, c_eps, c_div, c_sig),
                            int(seed), _key(sample0), _N, x.shape[1])

    def vpsde_purify(self, x0: torch.Tensor, c_a: float, c_b: float, k, h, hb, q, gs, z: Optional[torch.Tensor] = None, seed: int = 0,
                     sample0: int = 0, path: int = 0, want_traj: bool = False):
        """dmad_vpsde_purify: the reverse VP-SDE chain (diffusion to the start, then one Euler-Maruyama step per entry of k / h / hb /
        q / gs), one library call per chunk of max_batch clips.  path 0: the mode's default WaveNet path, 1: exact fp32.  z: optional
        explicit noise [S + 1, B, L] (slot 0 the diffusion draw, slot n + 1 step n); None = Philox keyed (seed, sample0 + row).
        want_traj: also return the trajectory for vpsde_purify_vjp, a [(S + 1) * B, L] tensor stored chunk by chunk: rows
        [(S + 1) * s, (S + 1) * e) hold the [S + 1][e - s][L] slots of the chunk [s, e)."""
        return self._vpsde_chain(self.lib.dmad_vpsde_purify, self._wave, self.L, x0, c_a, c_b, k, h, hb, q, gs, z, seed, sample0, path, want_traj)

    def vpsde_purify_vjp(self, traj: torch.Tensor, c_a: float, k, h, hb, q, g_out: torch.Tensor) -> torch.Tensor:
        """dmad_vpsde_purify_vjp: g_x0 = (d out / d x0)^T g_out of the chain vpsde_purify(.., path=1, want_traj=True) ran, the draws held
        fixed ([B, L] or [B, 1, L] -> [B, L]).  traj: that call's trajectory.  Needs reserve_vjp first (DmadError otherwise)."""
        return self._vpsde_chain_vjp(self.lib.dmad_vpsde_purify_vjp, self._wave, self.L, 'L', 'vpsde_purify', traj, c_a, k, h, hb, q, g_out)

    def _vpsde_chain(self, fn, shaper, width, x0, c_a, c_b, k, h, hb, q, gs, z, seed, sample0, path, want_traj):
        """vpsde_purify / spec_vpsde_purify: the library's chain `fn` on rows of `width` floats that `shaper` (_wave / _spec) checks."""
        x = shaper(x0)
        B, S = x.shape[0], len(k)
        out = torch.empty_like(x)
        traj = torch.empty(((S + 1) * B, width), dtype=torch.float32, device=x.device) if want_traj else None
        sched = self._vpsde_arrays(k, h, hb, q, gs)
        if z is not None:
            z = z.detach()
            if not z.is_cuda or tuple(z.shape) != (S + 1, B, width):
                raise DmadError('z must be a CUDA tensor [%d, %d, %d], not %s' % (S + 1, B, width, tuple(z.shape)))
            z = z.float()
        self._passes(fn, B, _per(x), _N, S, float(c_a), float(c_b), *sched, _cols(z), int(seed), _key(sample0), int(path), _per(out),
                     _per(traj, S + 1))
        return (out, traj) if want_traj else out

    def _vpsde_chain_vjp(self, fn, shaper, width, width_name, forward_name, traj, c_a, k, h, hb, q, g_out):
        """vpsde_purify_vjp / spec_vpsde_purify_vjp: the library's reverse walk `fn` over the chunk-by-chunk trajectory of `forward_name`."""
        g = shaper(g_out)
        B, S = g.shape[0], len(k)
        if not traj.is_cuda or tuple(traj.shape) != ((S + 1) * B, width):
            raise DmadError('traj must be the [(S + 1) * B, %s] = [%d, %d] trajectory of %s, not %s'
                            % (width_name, (S + 1) * B, width, forward_name, tuple(traj.shape)))
        gx = torch.empty_like(g)
        self._passes(fn, B, _per(traj, S + 1), _N, S, float(c_a), *self._vpsde_arrays(k, h, hb, q, h)[:4], _per(g), _per(gx))
        return gx

    @staticmethod
    def _vpsde_arrays(k, h, hb, q, gs):
        S = len(k)
        if not (len(h) == len(hb) == len(q) == len(gs) == S) or S < 1:
            raise DmadError('the schedule arrays k / h / hb / q / gs must have one entry per Euler step (%d)' % S)
        return [(C.c_int32 * S)(*[int(v) for v in k])] + _floats(S, h, hb, q, gs)

    # ------------------------------------------------------------------ mel front-end (and the masking loss on its STFT)
    def _mel(self, fn, x):
        x = self._wave(x)
        out = torch.empty((x.shape[0], 1, 32, 32), device=x.device, dtype=torch.float32)
        self._passes(fn, x.shape[0], _per(x), _N, _per(out))
        return out

    def mel_db(self, x: torch.Tensor) -> torch.Tensor:
        return self._mel(self.lib.dmad_mel_db, x)

    def mel_power(self, x: torch.Tensor) -> torch.Tensor:
        return self._mel(self.lib.dmad_mel_power, x)

    def power_to_db(self, x: torch.Tensor) -> torch.Tensor:
        _on_gpu(x)
        xc = _f32(x)
        out = torch.empty_like(xc)
        check(self.lib.dmad_power_to_db(self._h, _ptr(xc), xc.numel(), _ptr(out), _stream()))
        return out

    def mel_db_vjp(self, x: torch.Tensor, g_spec: torch.Tensor, want_spec: bool = False):
        """g_x = (d melDB / d x)^T g_spec for the dB mel front-end of mel_db ([B,1,L] or [B,L] -> [B,L]; g_spec [B,1,32,32] or [B,32,32]).
        want_spec: also return the spectrogram [B,1,32,32], bit-identical to mel_db(x).  The forward is recomputed; the first call
        allocates the workspace."""
        xw = self._wave(x)
        g = self._spec(g_spec)
        if g.shape[0] != xw.shape[0]:
            raise DmadError('g_spec has %d rows, x %d' % (g.shape[0], xw.shape[0]))
        gx = torch.empty_like(xw)
        sp = torch.empty((xw.shape[0], 1, 32, 32), device=xw.device, dtype=torch.float32) if want_spec else None
        self._passes(self.lib.dmad_mel_db_vjp, xw.shape[0], _per(xw), _N, _per(g), _per(gx), _per(sp))
        return (gx, sp) if want_spec else gx

    def masking_frames(self) -> int:
        """frames of torch.stft(n_fft=2048, hop_length=512, center=False) on a clip of this engine"""
        return (self.L - 2048) // 512 + 1

    def _masking_args(self, B, theta, psd_scale):
        F = self.masking_frames()
        _on_gpu(theta, psd_scale)
        if tuple(theta.shape) != (B, 1025, F) or psd_scale.numel() != B:
            raise DmadError('theta must be [%d, 1025, %d] and psd_scale [%d], not %s and %s'
                            % (B, F, B, tuple(theta.shape), tuple(psd_scale.shape)))
        return _f32(theta), psd_scale.detach().reshape(B).contiguous().float()

    def masking_loss_vjp(self, delta: torch.Tensor, theta: torch.Tensor, psd_scale: torch.Tensor, want_psd: bool = False):
        """dmad_masking_loss_vjp: the masking loss of the imperceptible attack and its gradient.  delta [B,1,L] or [B,L];
        theta [B,1025,F]: the stabilised threshold 10^(threshold / 10); psd_scale [B]: 10^9.6 / psd_maximum_stabilized.  Returns
        (g_delta [B,L], loss [B]) and, with want_psd, the normalised PSD estimate [B,1025,F]."""
        dw = self._wave(delta)
        B = dw.shape[0]
        th, sc = self._masking_args(B, theta, psd_scale)
        g = torch.empty_like(dw)
        loss = torch.empty((B,), device=dw.device, dtype=torch.float32)
        psd = torch.empty_like(th) if want_psd else None
        self._passes(self.lib.dmad_masking_loss_vjp, B, _per(dw), _N, _per(th), _per(sc), _per(g), _per(loss), _per(psd))
        return (g, loss, psd) if want_psd else (g, loss)

    def masking_step(self, x: torch.Tensor, delta: torch.Tensor, g_net: torch.Tensor, alpha: torch.Tensor, signed_lr: float,
                     theta: torch.Tensor, psd_scale: torch.Tensor) -> torch.Tensor:
        """dmad_masking_step: one update of stage 2, delta <- clamp(x + delta + signed_lr (g_net + alpha g_theta), -1, 1) - x IN PLACE
        (delta: a contiguous float32 CUDA tensor [B,1,L] or [B,L]; signed_lr = -lr targeted, +lr untargeted; alpha [B]).  Returns the
        masking loss [B] of delta before the update."""
        if not (delta.is_cuda and delta.dtype == torch.float32 and delta.is_contiguous()):
            raise DmadError('delta is updated in place: it must be a contiguous float32 tensor on the GPU (the dmad engine has no CPU path)')
        dw = self._wave(delta)
        assert dw.data_ptr() == delta.data_ptr()
        B = dw.shape[0]
        xw, gn = self._wave(x), self._wave(g_net)
        if xw.shape[0] != B or gn.shape[0] != B or alpha.numel() != B or not alpha.is_cuda:
            raise DmadError('x, g_net and alpha must hold %d rows on the GPU' % B)
        al = alpha.detach().reshape(B).contiguous().float()
        th, sc = self._masking_args(B, theta, psd_scale)
        loss = torch.empty((B,), device=dw.device, dtype=torch.float32)
        self._passes(self.lib.dmad_masking_step, B, _per(xw), _per(dw), _per(gn), _per(al), float(signed_lr), _N, _per(th), _per(sc), _per(loss))
        return loss

    # ------------------------------------------------------------------ UNet (the spectrogram-domain purifiers)
    def unet_eps(self, x_t: torch.Tensor, t: int, tier: Optional[int] = None) -> torch.Tensor:
        """eps = UNetModel(x_t, t * ones): [B,1,32,32] or [B,32,32] -> [B,32,32].  tier: None = the mode's tier of the map-returning
        surfaces (dmad_unet_eps); 0 exact fp32 / 1 16-bit / 2 split-f16 explicitly (dmad_unet_eps_tier)."""
        if tier is None:
            return self._mapped(self.lib.dmad_unet_eps, self._spec(x_t), int(t), _N)
        return self._mapped(self.lib.dmad_unet_eps_tier, self._spec(x_t), int(t), _N, int(tier))

    def unet_p_sample(self, x: torch.Tensor, t: int, c_a: float, c_b: float, c_1: float, c_2: float, c_sig: float,
                      z: Optional[torch.Tensor] = None, seed: int = 0, sample0: int = 0, want_x0: bool = False):
        """in place on x ([B,32,32] contiguous fp32 CUDA); returns pred_xstart when asked."""
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and tuple(x.shape[1:]) == (32, 32)
        x0 = torch.empty_like(x) if want_x0 else None
        zz = None if z is None else self._spec(z)
        self._passes(self.lib.dmad_unet_p_sample, x.shape[0], _per(x), int(t), float(c_a), float(c_b), float(c_1), float(c_2), float(c_sig),
                     _per(zz), int(seed), _key(sample0), _N, _per(x0))
        return x0

    def reserve_unet_vjp(self, max_batch: int):
        """dmad_reserve_unet_vjp: the workspace of unet_eps_vjp (the forward's tape) for up to max_batch spectrograms per pass (capped at
        the engine's fp32 pass size; a larger reservation replaces a smaller one).  FP32 / EXACT engines; DmadError otherwise."""
        self._reserve('unet_vjp', max_batch)

    def unet_eps_vjp(self, x_t: torch.Tensor, t: int, g_eps: torch.Tensor, want_eps: bool = False):
        """g_x = (d eps / d x_t)^T g_eps for eps = UNetModel(x_t, t * ones) on the exact-fp32 tier ([B,1,32,32] or [B,32,32] -> [B,32,32]).
        want_eps: also return eps, bit-identical to unet_eps(x_t, t, tier=0).  Needs reserve_unet_vjp first (DmadError otherwise)."""
        return self._eps_vjp(self.lib.dmad_unet_eps_vjp, self._spec, x_t, t, g_eps, want_eps)

    def spec_vpsde_purify(self, x0: torch.Tensor, c_a: float, c_b: float, k, h, hb, q, gs, z: Optional[torch.Tensor] = None, seed: int = 0,
                          sample0: int = 0, path: int = 0, want_traj: bool = False):
        """dmad_spec_vpsde_purify: vpsde_purify's chain on standardised spectrograms with the UNet as the eps-network ([B,1,32,32] or
        [B,32,32] -> [B,32,32]), one library call per chunk of max_batch.  path 0: the mode's UNet map tier (unet_eps(tier=None)), 1: exact
        fp32.  z: optional explicit noise [S + 1, B, 1024]; None = Philox keyed (seed, sample0 + row).  want_traj: also return the
        trajectory for spec_vpsde_purify_vjp, [(S + 1) * B, 1024] stored chunk by chunk as in vpsde_purify."""
        return self._vpsde_chain(self.lib.dmad_spec_vpsde_purify, self._spec, 1024, x0, c_a, c_b, k, h, hb, q, gs, z, seed, sample0, path, want_traj)

    def spec_vpsde_purify_vjp(self, traj: torch.Tensor, c_a: float, k, h, hb, q, g_out: torch.Tensor) -> torch.Tensor:
        """dmad_spec_vpsde_purify_vjp: g_x0 = (d out / d x0)^T g_out of the chain spec_vpsde_purify(.., path=1, want_traj=True) ran, the
        draws held fixed ([B,1,32,32] or [B,32,32] -> [B,32,32]).  traj: that call's trajectory.  Needs reserve_unet_vjp first."""
        return self._vpsde_chain_vjp(self.lib.dmad_spec_vpsde_purify_vjp, self._spec, 1024, '1024', 'spec_vpsde_purify', traj, c_a, k, h, hb, q, g_out)

    # ------------------------------------------------------------------ spectrogram classifiers (VGG19_bn / ResNeXt29)
    def _classify(self, fn, spec, *tier):
        _on_gpu(spec)
        sp = spec.detach().reshape(spec.shape[0], 32 * 32).contiguous().float()
        out = torch.empty((sp.shape[0], self.num_classes), device=sp.device, dtype=torch.float32)
        self._passes(fn, sp.shape[0], _per(sp), _N, *tier, _per(out))
        return out

    def classify(self, spec: torch.Tensor) -> torch.Tensor:
        return self._classify(self.lib.dmad_classify, spec)

    def classify_tier(self, spec: torch.Tensor, tier: int) -> torch.Tensor:
        """dmad_classify_tier: the classifier on an explicit tier (0 fp32, 1 the 16-bit tier / 2 the split-f16 tier of ResNeXt29) — test / measurement hook."""
        return self._classify(self.lib.dmad_classify_tier, spec, int(tier))

    def reserve_classifier_vjp(self, max_batch: int):
        """dmad_reserve_classifier_vjp: the workspace of classify_vjp (the ResNeXt29 forward's tape) for up to max_batch spectrograms per
        pass (capped at max_batch; a larger reservation replaces a smaller one).  ResNeXt29 engines of every precision; DmadError otherwise."""
        self._reserve('classifier_vjp', max_batch)

    def _logits_vjp(self, fn, spec, g_logits, want_logits, reserve=None):
        """classify_vjp / vgg_vjp: the export `fn`; reserve: called with B when no workspace is reserved yet (vgg_vjp)"""
        sp = self._spec(spec)
        B = sp.shape[0]
        if not g_logits.is_cuda or tuple(g_logits.shape) != (B, self.num_classes):
            raise DmadError('g_logits must be a CUDA tensor [%d, %d], not %s' % (B, self.num_classes, tuple(g_logits.shape)))
        if reserve is not None:
            reserve(B)
        g = _f32(g_logits)
        gs = torch.empty_like(sp)
        lg = torch.empty((B, self.num_classes), device=sp.device, dtype=torch.float32) if want_logits else None
        self._passes(fn, B, _per(sp), _N, _per(g), _per(gs), _per(lg))
        return (gs, lg) if want_logits else gs

    def classify_vjp(self, spec: torch.Tensor, g_logits: torch.Tensor, want_logits: bool = False):
        """g_spec = (d logits / d spec)^T g_logits for logits = CifarResNeXt(spec) on the fp32 tier ([B,1,32,32] or [B,32,32] -> [B,32,32]).
        want_logits: also return the logits, bit-identical to classify_tier(spec, 0).  Needs reserve_classifier_vjp first (DmadError
        otherwise); ResNeXt29 engines only."""
        return self._logits_vjp(self.lib.dmad_classify_vjp, spec, g_logits, want_logits)

    def reserve_vgg_vjp(self, max_batch: int):
        """dmad_reserve_vgg_vjp: the workspace of vgg_vjp (the VGG19_bn forward's tape, the gradient maps and, once, the backward weight
        images) for up to max_batch spectrograms per pass (capped at max_batch; a larger reservation replaces a smaller one).  VGG19_bn
        engines of every precision; DmadError otherwise."""
        self._reserve('vgg_vjp', max_batch, min(int(max_batch), self.max_batch))

    def vgg_vjp(self, spec: torch.Tensor, g_logits: torch.Tensor, want_logits: bool = False):
        """g_spec = (d logits / d spec)^T g_logits for logits = VGG19_bn(spec) on the fp32 tier ([B,1,32,32] or [B,32,32] -> [B,32,32]).
        want_logits: also return the logits, bit-identical to classify_tier(spec, 0).  Without a reservation the first call reserves
        its own rows (capped at max_batch); a present reservation is kept and a larger call runs in passes of its size, with the same
        bits (reserve_vgg_vjp chooses the pass size; autograd.VGGHIP grows it to the batch it meets).  VGG19_bn engines only."""
        return self._logits_vjp(self.lib.dmad_vgg_vjp, spec, g_logits, want_logits, None if self.vgg_vjp_batch else self.reserve_vgg_vjp)

    def vgg_vjp_tape(self, index: int, B: int) -> torch.Tensor:
        """dmad_vgg_vjp_tape: map `index` of the last vgg_vjp call's tape, rows [0, B) — 0 - 15 the post-ReLU conv maps [B,H,H,C] (NHWC),
        16 - 17 the post-ReLU FC vectors [B,4096] (test hook; that call must have run as one pass)."""
        if index < 16:
            H, C = VGG_TAPE_MAPS[index]
            out = torch.empty((int(B), H, H, C), device='cuda', dtype=torch.float32)
        else:
            out = torch.empty((int(B), 4096), device='cuda', dtype=torch.float32)
        check(self.lib.dmad_vgg_vjp_tape(self._h, int(index), int(B), _ptr(out), _stream()))
        return out

    def reserve_wrn_vjp(self, max_batch: int):
        """dmad_reserve_wrn_vjp: the workspace of wrn_vjp (the WideResNet forward's tape of 25 post-ReLU maps, the gradient maps and, once,
        the backward weight images) for up to max_batch spectrograms per pass (capped at max_batch; a larger reservation replaces a
        smaller one).  WideResNet engines of every precision; DmadError otherwise."""
        self._reserve('wrn_vjp', max_batch, min(int(max_batch), self.max_batch))

    def wrn_vjp(self, spec: torch.Tensor, g_logits: torch.Tensor, want_logits: bool = False):
        """g_spec = (d logits / d spec)^T g_logits for logits = WideResNet-28-10(spec) on the fp32 tier ([B,1,32,32] or [B,32,32] ->
        [B,32,32]).  want_logits: also return the logits, bit-identical to classify_tier(spec, 0).  Reserves on demand like vgg_vjp."""
        return self._logits_vjp(self.lib.dmad_wrn_vjp, spec, g_logits, want_logits, None if self.wrn_vjp_batch else self.reserve_wrn_vjp)

    def wrn_vjp_tape(self, index: int, B: int) -> torch.Tensor:
        """dmad_wrn_vjp_tape: map `index` (0..24, WRN_TAPE_MAPS) of the last wrn_vjp call's tape, rows [0, B), NHWC [B,H,H,C] (test hook;
        that call must have run as one pass)."""
        if not 0 <= int(index) < len(WRN_TAPE_MAPS):
            raise DmadError('tape map %d outside [0, %d]' % (index, len(WRN_TAPE_MAPS) - 1))
        H, Cn = WRN_TAPE_MAPS[index]
        out = torch.empty((int(B), H, H, Cn), device='cuda', dtype=torch.float32)
        check(self.lib.dmad_wrn_vjp_tape(self._h, int(index), int(B), _ptr(out), _stream()))
        return out

    def reserve_dn_vjp(self, max_batch: int):
        """dmad_reserve_dn_vjp: the workspace of dn_vjp (the DenseNet forward's tape: the three streams and the 48 h maps; the gradient
        streams) for up to max_batch spectrograms per pass (capped at max_batch; a larger reservation replaces a smaller one).  DenseNet
        engines of every precision; DmadError otherwise."""
        self._reserve('dn_vjp', max_batch, min(int(max_batch), self.max_batch))

    def dn_vjp(self, spec: torch.Tensor, g_logits: torch.Tensor, want_logits: bool = False):
        """g_spec = (d logits / d spec)^T g_logits for logits = DenseNet-BC-100-12(spec) on the fp32 tier ([B,1,32,32] or [B,32,32] ->
        [B,32,32]).  want_logits: also return the logits, bit-identical to classify_tier(spec, 0).  Reserves on demand like vgg_vjp."""
        return self._logits_vjp(self.lib.dmad_dn_vjp, spec, g_logits, want_logits, None if self.dn_vjp_batch else self.reserve_dn_vjp)

    def dn_vjp_tape(self, index: int, B: int) -> torch.Tensor:
        """dmad_dn_vjp_tape: post-ReLU map `index` (0..98, DN_TAPE_MAPS) of the last dn_vjp call's forward, rows [0, B), NHWC [B,H,H,C]
        (test hook; that call must have run as one pass)."""
        if not 0 <= int(index) < len(DN_TAPE_MAPS):
            raise DmadError('tape map %d outside [0, %d]' % (index, len(DN_TAPE_MAPS) - 1))
        H, Cn = DN_TAPE_MAPS[index]
        out = torch.empty((int(B), H, H, Cn), device='cuda', dtype=torch.float32)
        check(self.lib.dmad_dn_vjp_tape(self._h, int(index), int(B), _ptr(out), _stream()))
        return out

    # ------------------------------------------------------------------ the vote loops and their exact-vote mode (EXACT engines)
    def vote(self, logits: torch.Tensor, counts: torch.Tensor):
        lg = logits.detach().contiguous().float()
        assert lg.is_cuda and counts.is_cuda and counts.dtype == torch.int64 and lg.shape[1] == self.num_classes
        check(self.lib.dmad_vote(self._h, _ptr(lg), lg.shape[0], _ptr(counts), _stream()))

    def _vote_state(self, clip, batch, counts):
        """smooth_votes / spec_smooth_votes: the clip, the pass size (at most max_batch) and the counts to add to"""
        clip = self._clip(clip)
        if counts is None:
            counts = torch.zeros(self.num_classes, dtype=torch.int64, device=clip.device)
        return clip, min(batch or self.max_batch, self.max_batch), counts

    def smooth_votes(self, clip: torch.Tensor, sigma: float, sqrt_abar_star: float, t: int, c_a: float, c_b: float,
                     n: int, batch: Optional[int] = None, seed: int = 0, sample0: int = 0,
                     delta: Optional[torch.Tensor] = None, want_logits: bool = False, want_x0: bool = False,
                     counts: Optional[torch.Tensor] = None):
        """The fused Monte Carlo loop (dmad_smooth_votes).  Returns (counts[int64, C] on device, logits|None, x0|None)."""
        clip, batch, counts = self._vote_state(clip, batch, counts)
        logits = torch.empty((n, self.num_classes), device=clip.device) if want_logits else None
        x0 = torch.empty((n, self.L), device=clip.device) if want_x0 else None
        if delta is not None:
            delta = delta.detach().reshape(n, self.L).contiguous().float()
            assert delta.is_cuda
        check(self.lib.dmad_smooth_votes(self._h, _ptr(clip), float(sigma), float(sqrt_abar_star), int(t), float(c_a), float(c_b),
                                         int(n), int(batch), int(seed), int(sample0), _ptr(delta), _ptr(counts), _ptr(logits),
                                         _ptr(x0), _stream()))
        return counts, logits, x0

    def _noise_rows(self, delta: Optional[torch.Tensor], n: int) -> Optional[torch.Tensor]:
        """the caller's noise of a randomized-smoothing loop as [n, L] float32 on the device"""
        if delta is None:
            return None
        delta = delta.detach().reshape(n, self.L).contiguous().float()
        assert delta.is_cuda
        return delta if delta.data_ptr() % 16 == 0 else delta.clone()         # the kernels read 16 bytes at a time

    def rs_smooth_votes(self, clip: torch.Tensor, sigma: float, n: int, batch: Optional[int] = None, seed: int = 0, sample0: int = 0,
                        delta: Optional[torch.Tensor] = None, want_logits: bool = False, counts: Optional[torch.Tensor] = None):
        """dmad_rs_smooth_votes: the Monte Carlo loop without a purifier (RobustCertificate with denoiser=None) in one call: clip + noise
        -> mel dB -> the classifier's fp32 tier -> votes.  Returns (counts[int64, C] on device, logits|None), bit for bit what
        classify(mel_db(clip + sigma * philox_normal(seed, sample0, 0, n))) and vote give."""
        clip, batch, counts = self._vote_state(clip, batch, counts)
        if clip.data_ptr() % 16:
            clip = clip.clone()
        logits = torch.empty((n, self.num_classes), device=clip.device) if want_logits else None
        delta = self._noise_rows(delta, n)
        check(self.lib.dmad_rs_smooth_votes(self._h, _ptr(clip), float(sigma), int(n), int(batch), int(seed), int(sample0), _ptr(delta),
                                            _ptr(counts), _ptr(logits), _stream()))
        return counts, logits

    def eval_samples(self, clip: torch.Tensor, sigma: float, sqrt_abar_star: float, t: int, c_a: float, c_b: float,
                     idx: torch.Tensor, path: int = 0, seed: int = 0, sample0: int = 0, delta: Optional[torch.Tensor] = None,
                     want_x0: bool = False):
        """dmad_eval_samples: logits [len(idx), C] (and x0 [len(idx), L] when asked) of the Monte Carlo samples with GLOBAL indices
        `idx` (int64, device) on WaveNet path 0 (the mode's default) / 1 (exact fp32) / 2 (split-f16).  Nothing votes."""
        clip = self._clip(clip)
        idx = idx.detach().to(device=clip.device, dtype=torch.int64).contiguous()
        n = idx.numel()
        logits = torch.empty((n, self.num_classes), device=clip.device)
        x0 = torch.empty((n, self.L), device=clip.device) if want_x0 else None
        if delta is not None:
            delta = delta.detach().reshape(-1, self.L).contiguous().float()
            assert delta.is_cuda
        check(self.lib.dmad_eval_samples(self._h, _ptr(clip), float(sigma), float(sqrt_abar_star), int(t), float(c_a), float(c_b),
                                         int(seed), int(sample0), _ptr(delta), _ptr(idx), int(n), int(path), _ptr(logits), _ptr(x0),
                                         _stream()))
        return (logits, x0) if want_x0 else logits

    def spec_smooth_votes(self, clip: torch.Tensor, sigma: float, t_star: int, q_a: float, q_b: float, c_a, c_b, c_1, c_2, c_sig,
                          mel_lo: float, mel_hi: float, n: int, batch: Optional[int] = None, seed: int = 0, sample0: int = 0,
                          want_logits: bool = False, want_spec: bool = False, counts: Optional[torch.Tensor] = None):
        """dmad_spec_smooth_votes (BASELINE C5): the vote loop with the spec-domain UNet purifier.  Coefficient sequences
        c_*: t_star + 1 floats each (p_sample at t = 0..t_star).  Returns (counts, logits|None, purified spec|None)."""
        clip, batch, counts = self._vote_state(clip, batch, counts)
        logits = torch.empty((n, self.num_classes), device=clip.device) if want_logits else None
        spec = torch.empty((n, 1, 32, 32), device=clip.device) if want_spec else None
        check(self.lib.dmad_spec_smooth_votes(self._h, _ptr(clip), float(sigma), int(t_star), float(q_a), float(q_b),
                                              *_floats(t_star + 1, c_a, c_b, c_1, c_2, c_sig), float(mel_lo), float(mel_hi), int(n), int(batch),
                                              int(seed), int(sample0), _ptr(counts), _ptr(logits), _ptr(spec), _stream()))
        return counts, logits, spec

    def spec_eval_samples(self, clip: torch.Tensor, sigma: float, t_star: int, q_a: float, q_b: float, c_a, c_b, c_1, c_2, c_sig,
                          mel_lo: float, mel_hi: float, idx: torch.Tensor, tier: int, seed: int = 0, want_spec: bool = False):
        """dmad_spec_eval_samples: logits [len(idx), C] (and the purified dB spectrograms when asked) of the spec-domain chain for
        the Monte Carlo samples with GLOBAL indices `idx` on UNet tier 0 (exact fp32) / 1 (16-bit) / 2 (split-f16).  Nothing votes."""
        clip = self._clip(clip)
        idx = idx.detach().to(device=clip.device, dtype=torch.int64).contiguous()
        n = idx.numel()
        logits = torch.empty((n, self.num_classes), device=clip.device)
        spec = torch.empty((n, 1, 32, 32), device=clip.device) if want_spec else None
        check(self.lib.dmad_spec_eval_samples(self._h, _ptr(clip), float(sigma), int(t_star), float(q_a), float(q_b),
                                              *_floats(t_star + 1, c_a, c_b, c_1, c_2, c_sig), float(mel_lo), float(mel_hi), int(seed), _ptr(idx),
                                              int(n), int(tier), _ptr(logits), _ptr(spec), _stream()))
        return (logits, spec) if want_spec else logits

    def set_mode(self, mode: int):
        check(self.lib.dmad_set_mode(self._h, int(mode)))
        self.mode = int(mode)

    def set_waveform_tier(self, tier: int):
        """dmad_set_waveform_tier: WaveNet tier of the waveform-returning surfaces (wavenet_eps, one_shot, ddpm_step / purify, the purifier
        inside query_logits) of an exact-vote engine: WAVE_SPLIT (default: fp32-grade, 8e-5), WAVE_FP32, WAVE_16BIT (4e-3)."""
        check(self.lib.dmad_set_waveform_tier(self._h, int(tier)))
        self.waveform_tier = int(tier)

    def _set_margin(self, setter, attr: str, floor_attr: str, committed: float, tau: float, calibrated: bool):
        """the four margin setters (the floor rule: set_recheck_margin)"""
        check(setter(self._h, float(tau)))
        setattr(self, attr, float(tau))
        if not calibrated:
            setattr(self, floor_attr, max(committed, float(tau)))

    def set_recheck_margin(self, tau: float, calibrated: bool = False):
        """bound of the 16-bit tier.  A value the CALLER sets (calibrated = False) also becomes the floor of later calibrations when it
        is wider than the committed default: a calibration may only widen what is in force."""
        self._set_margin(self.lib.dmad_set_recheck_margin, 'recheck_margin', 'floor1', self._committed_margin1(), tau, calibrated)

    def _committed_margin1(self) -> float:
        """the committed tier-1 bound for this engine's operand format and resident classifier kind"""
        kind = getattr(self, 'classifier_kind', None)
        if kind == 'wideresnet28_10':
            raise DmadError('no recheck bound has been measured for WideResNet-28-10: it has no committed margin')
        if kind == 'densenet_bc_100_12':
            raise DmadError('no recheck bound has been measured for DenseNet-BC-100-12: it has no committed margin')
        table = DEFAULT_RECHECK_MARGIN_RESNEXT29 if kind == 'resnext29' else DEFAULT_RECHECK_MARGIN
        return table[self.half_type]

    def set_recheck_margin2(self, tau2: float, calibrated: bool = False):
        """bound of the split-f16 middle tier (< 0: tier off, queued samples go straight to the fp32 path)."""
        self._set_margin(self.lib.dmad_set_recheck_margin2, 'recheck_margin2', 'floor2', DEFAULT_RECHECK_MARGIN2, tau2, calibrated)

    def set_spec_recheck_margin(self, tau: float, calibrated: bool = False):
        """bound of the spec-domain vote loop's 16-bit UNet tier (dmad_set_spec_recheck_margin)."""
        self._set_margin(self.lib.dmad_set_spec_recheck_margin, 'spec_recheck_margin', 'floor_spec', DEFAULT_SPEC_RECHECK_MARGIN, tau, calibrated)

    def set_spec_recheck_margin2(self, tau2: float, calibrated: bool = False):
        """bound of the spec-domain loop's split-f16 UNet tier (dmad_set_spec_recheck_margin2); < 0: queued samples go straight to fp32."""
        self._set_margin(self.lib.dmad_set_spec_recheck_margin2, 'spec_recheck_margin2', 'floor_spec2', DEFAULT_SPEC_RECHECK_MARGIN2, tau2,
                         calibrated)

    def _stats(self, fn, reset, detail):
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(fn(self._h, C.byref(a), C.byref(b), C.byref(c), 1 if reset else 0))
        return (int(a.value), int(b.value), int(c.value)) if detail else (int(a.value), int(b.value))

    def recheck_stats(self, reset: bool = False, detail: bool = False):
        """-> (samples voted, samples that left the 16-bit pass) since the last reset; detail: + samples that reached fp32."""
        return self._stats(self.lib.dmad_recheck_stats, reset, detail)

    def spec_recheck_stats(self, reset: bool = False, detail: bool = False):
        """-> (samples voted by spec_smooth_votes, samples whose chain left the 16-bit tier) since the last reset; detail: + the samples
        that reached the exact-fp32 UNet."""
        return self._stats(self.lib.dmad_spec_recheck_stats2, reset, detail)

    def _measure_tiers(self, what: str, clips: list, n: int, n_fp32: int, seed: int, tiers: list):
        """The measurement behind both loops' calibrations.  tiers = evaluators (clip, idx, seed) -> logits of the loop's first pass, its
        split-f16 tier and its exact-fp32 tier; per clip (seed + its position) n Philox samples run on the first two, the first n_fp32 of
        them on the third, in the exact-vote mode (the first pass's classifier tier depends on the mode).  Returns (e1, s1, e2): the largest
        leader-difference error of the first pass against the split-f16 tier, its Gaussian scale, and the largest error of the split-f16
        tier against fp32, each the maximum over the clips."""
        if self.precision != EXACT:
            raise DmadError('%s needs an EXACT engine' % what)

        def lead_err(a, ref):                # per-sample error of a logit difference against the reference's leader (see DEFAULT_RECHECK_MARGIN)
            d = a - ref
            return (d - d.gather(1, ref.argmax(1, keepdim=True))).abs().max(1).values

        def gauss_scale(le):                 # P(max of 9 |normal differences| > x) ~= 18 Q(x / s): s from the q90 and q99 points
            zs = {0.9: 2.5392, 0.99: 3.2608}            # 18 Q(z) = 1 - q
            return max(float(torch.quantile(le, q)) / z for q, z in zs.items())
        e1 = s1 = e2 = 0.0
        mode = self.mode
        self.set_mode(MODE_EXACT_VOTES)
        try:
            for ci, x in enumerate(clips):
                idx = torch.arange(n, dtype=torch.int64, device=self.device)
                lo, mid, ref = (f(x, i, seed + ci) for f, i in zip(tiers, (idx, idx, idx[:n_fp32])))
                if not all(bool(torch.isfinite(v).all()) for v in (lo, mid, ref)):
                    raise DmadError('%s: non-finite logits' % what)
                le1 = lead_err(lo.double(), mid.double())
                e1, s1 = max(e1, float(le1.max())), max(s1, gauss_scale(le1))
                e2 = max(e2, float(lead_err(mid[:n_fp32].double(), ref.double()).max()))
        finally:
            self.set_mode(mode)
        return e1, s1, e2

    @staticmethod
    def _widened(floor1: float, floor2: float, headroom: float, e1: float, s1: float, e2: float):
        """the bound rule of both calibrations (calibrate_recheck's docstring): -> (first-pass bound, split-f16 tier's bound), widen-only"""
        new2 = max(floor2, headroom * e2)
        return max(floor1, headroom * e1 + new2, TAIL_Z * s1 + new2), new2

    def calibrate_recheck(self, clip, sigma: float, sqrt_abar_star: float, t: int, c_a: float, c_b: float,
                          n: int = 1024, n_fp32: int = 512, headroom: float = 1.5, seed: int = 0xCA11B):
        """Measure, for THE RESIDENT WEIGHTS, what the defaults were measured for on the synthetic VGG19_bn (see
        DEFAULT_RECHECK_MARGIN): the largest error the 16-bit pass makes on a logit difference against the leader (vs the split-f16
        tier, n Philox samples per clip at this sigma) and the largest error of the split-f16 tier (against the exact-fp32 path,
        n_fp32 samples per clip).  `clip`: one clip or a list of clips (the maxima are taken over all of them).  The bounds become
            tau2 = max(committed default, headroom * e2),
            tau1 = max(committed default, headroom * e1 + tau2, TAIL_Z * s1 + tau2),
        s1 = the Gaussian scale of the per-sample error statistic read off its upper quantiles (q90, q99 of max_j |e_j - e_i|
        ~ the maximum of 9 normal differences): TAIL_Z * s1 is where the tail model of tools/fit_recheck_tail.py puts the
        per-sample miss probability at 1e-9 (on the committed study: 5.4 x 0.0056 = 0.030 < 0.034).
        A calibration can only WIDEN a bound — a maximum over a few hundred samples underestimates the tail the committed
        defaults were derived from (36 864 samples), so it is never allowed to go below them.  The logit sensitivity of a
        classifier — hence the error a given eps error turns into — is a property of its weights: call this once per
        (WaveNet, classifier, sigma) before certifying with checkpoints other than the ones the defaults were measured on.
        Returns (tau1, tau2, e1, e2); the observed errors are also kept in self.calibration."""
        clips = list(clip) if isinstance(clip, (list, tuple)) else [clip]
        tau1, tau2 = self.recheck_margin, self.recheck_margin2
        n_fp32 = min(n_fp32, n)

        def path(p):                         # path 0 in the exact-vote mode = the loop's FIRST PASS: 16-bit WaveNet + the classifier tier it runs
            return lambda x, idx, sd: self.eval_samples(x, sigma, sqrt_abar_star, t, c_a, c_b, idx, path=p, seed=sd)
        e1, s1, e2 = self._measure_tiers('calibrate_recheck', clips, n, n_fp32, seed, [path(0), path(2), path(1)])
        floor1, floor2 = self.floor1, self.floor2         # the committed defaults, or a wider bound the caller put in force
        new1, new2 = self._widened(floor1, floor2, headroom, e1, s1, e2)
        self.set_recheck_margin(new1, calibrated=True); self.set_recheck_margin2(new2, calibrated=True)
        self.calibration = {'e1': e1, 'e2': e2, 's1': s1, 'tau1': new1, 'tau2': new2, 'n': n, 'n_fp32': n_fp32, 'clips': len(clips),
                            'headroom': headroom, 'floor1': floor1, 'floor2': floor2,
                            'previous': (tau1, tau2)}
        return new1, new2, e1, e2

    def calibrate_spec_recheck(self, clip, sigma: float, chain_args: tuple, n: int = 256, headroom: float = 1.5, seed: int = 0x5BECCA1,
                               n_fp32: Optional[int] = None):
        """The spec-domain counterpart of calibrate_recheck: for THE RESIDENT WEIGHTS and this (sigma, t*), run n Monte Carlo samples'
        whole chains per clip on the UNet's 16-bit tier and on its split-f16 tier, and the first n_fp32 (default n / 2) of them on the
        exact-fp32 tier, from the same Philox keys; take the leader-difference error statistic (see DEFAULT_RECHECK_MARGIN) and set
            tau_spec2 = max(floor2, headroom * e2)                                    (split-f16 tier against fp32)
            tau_spec  = max(floor, headroom * e + tau_spec2, TAIL_Z * s + tau_spec2)  (16-bit tier against the split-f16 tier)
        with e its largest value and s its Gaussian scale (q90 / q99 points), floors = the committed defaults (or wider bounds the
        caller put in force): widen-only.  chain_args = (t_star, q_a, q_b, c_a, c_b, c_1, c_2, c_sig, mel_lo, mel_hi) as for
        spec_smooth_votes.  Returns (tau_spec, e, s); the full record is kept in self.spec_calibration."""
        clips = list(clip) if isinstance(clip, (list, tuple)) else [clip]
        n_fp32 = max(1, min(n, n // 2 if n_fp32 is None else n_fp32))

        def tier(k):
            return lambda x, idx, sd: self.spec_eval_samples(x, sigma, *chain_args, idx, tier=k, seed=sd)
        e, s, e2 = self._measure_tiers('calibrate_spec_recheck', clips, n, n_fp32, seed, [tier(1), tier(2), tier(0)])
        previous, floor, floor2 = (self.spec_recheck_margin, self.spec_recheck_margin2), self.floor_spec, self.floor_spec2
        new, new2 = self._widened(floor, floor2, headroom, e, s, e2)
        self.set_spec_recheck_margin(new, calibrated=True); self.set_spec_recheck_margin2(new2, calibrated=True)
        self.spec_calibration = {'e': e, 's': s, 'e2': e2, 'tau_spec': new, 'tau_spec2': new2, 'n': n, 'n_fp32': n_fp32, 'clips': len(clips),
                                 'headroom': headroom, 'floor': floor, 'floor2': floor2, 'previous': previous, 'sigma': sigma,
                                 't_star': int(chain_args[0])}
        return new, e, s

    def debug_rounding(self, dil: int = 0, res: int = 0, skip: int = 0, f0: int = 0, init: int = 0):
        """dmad_debug_rounding (measurement hook): single roundings of the 16-bit path switched on inside the split-f16 tier."""
        m = (C.c_int32 * 5)(int(dil), int(res), int(skip), int(f0), int(init))
        check(self.lib.dmad_debug_rounding(self._h, m))

    # ------------------------------------------------------------------ the query surfaces of the black-box attacks
    def _query(self, fn, width, x, repeats, sampler, t_star, c_a, c_b, c_eps, c_div, c_sig, seed, sample0):
        """query_logits / m5_query_logits: the export `fn`, whose logits are `width` wide"""
        xw = self._wave(x)
        B = xw.shape[0]
        logits, dec = self._logits_pair(repeats * B, width, xw.device)
        arrs = _floats(t_star, c_eps, c_div, c_sig) if sampler == 1 else [None, None, None]
        check(fn(self._h, _ptr(xw), B, int(repeats), int(sampler), int(t_star), float(c_a), float(c_b), *arrs, int(seed), int(sample0),
                 _ptr(logits), _ptr(dec), _stream()))
        return logits, dec

    def query_logits(self, x: torch.Tensor, repeats: int, sampler: int = 0, t_star: int = 0, c_a: float = 0.0, c_b: float = 0.0,
                     c_eps=None, c_div=None, c_sig=None, seed: int = 0, sample0: int = 0):
        """dmad_query_logits: x [B,1,L] -> (logits [repeats*B, C], decisions int32 [repeats*B]); row r*B+b is clip b."""
        return self._query(self.lib.dmad_query_logits, self.num_classes, x, repeats, sampler, t_star, c_a, c_b, c_eps, c_div, c_sig, seed, sample0)

    def spec_query_logits(self, x: torch.Tensor, repeats: int, t_star: int, q_a: float, q_b: float, c_a, c_b, c_1, c_2, c_sig,
                          mel_lo: float, mel_hi: float, seed: int = 0, sample0: int = 0):
        """dmad_spec_query_logits: x [B,1,L] -> (logits [repeats*B, C], decisions int32 [repeats*B]) through the spec-domain chain
        (mel dB -> standardise -> q_sample(t*) -> p_sample steps -> un-standardise -> classifier); row r*B+b is clip b."""
        xw = self._wave(x)
        B = xw.shape[0]
        logits, dec = self._logits_pair(repeats * B, self.num_classes, xw.device)
        check(self.lib.dmad_spec_query_logits(self._h, _ptr(xw), B, int(repeats), int(t_star), float(q_a), float(q_b),
                                              *_floats(t_star + 1, c_a, c_b, c_1, c_2, c_sig), float(mel_lo), float(mel_hi), int(seed), int(sample0),
                                              _ptr(logits), _ptr(dec), _stream()))
        return logits, dec

    # ------------------------------------------------------------------ NES probes and the particle swarm (FAKEBOB, SirenAttack)
    def nes_probes(self, x: torch.Tensor, P: int, sigma: float, with_origin: bool, seed: int = 0, draw0: int = 0, row0: int = 0,
                   rows: Optional[int] = None) -> torch.Tensor:
        """dmad_nes_probes: x [B,1,L] -> query rows [row0, row0 + rows) of the NES layout, [rows, L] (clip-major, P + with_origin rows per
        clip: x[b], then x[b] + sigma * u_j, then x[b] - sigma * u_j; u_j = philox_normal(seed, draw0 + b * P/2 + j, NES_STREAM, 1)).
        rows defaults to all that follow row0."""
        xw = self._wave(x)
        B = xw.shape[0]
        if rows is None:
            rows = B * (int(P) + int(bool(with_origin))) - int(row0)
        out = torch.empty((max(int(rows), 0), self.L), device=xw.device, dtype=torch.float32)
        check(self.lib.dmad_nes_probes(self._h, _ptr(xw), B, int(P), float(sigma), int(bool(with_origin)), int(seed), int(draw0), int(row0),
                                       int(rows), _ptr(out), _stream()))
        return out

    def nes_grad(self, w: torch.Tensor, P: int, scale: float, seed: int = 0, draw0: int = 0, grad: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dmad_nes_grad: w [B, P] probe losses (+ probes first) -> scale * sum_j (w[b][j] - w[b][P/2 + j]) u_{b,j}, [B, L], the directions
        regenerated on the device.  With `grad` ([B, L] contiguous fp32 CUDA) the estimate is added to it in place."""
        _on_gpu(w)
        w = _f32(w)
        assert w.dim() == 2 and w.shape[1] == int(P), 'expected w [B,%d], got %s' % (int(P), tuple(w.shape))
        B = w.shape[0]
        accumulate = grad is not None
        if accumulate:
            assert grad.is_cuda and grad.is_contiguous() and grad.dtype == torch.float32 and tuple(grad.shape) == (B, self.L)
        else:
            grad = torch.empty((B, self.L), device=w.device, dtype=torch.float32)
        check(self.lib.dmad_nes_grad(self._h, _ptr(w), B, int(P), float(scale), int(seed), int(draw0), int(accumulate), _ptr(grad), _stream()))
        return grad

    def _owned(self, t: Optional[torch.Tensor], shape, dtype=torch.float32, name='state') -> torch.Tensor:
        """A caller-owned tensor a swarm call updates in place: checked, never copied; None -> a new one."""
        if t is None:
            return torch.empty(shape, device=self.device, dtype=dtype)
        _on_gpu(t)
        assert t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == tuple(shape), \
            '%s: expected contiguous %s %s, got %s %s' % (name, dtype, tuple(shape), t.dtype, tuple(t.shape))
        return t

    def pso_init(self, x: torch.Tensor, lower: torch.Tensor, upper: torch.Tensor, P: int, seed: int = 0, draw0: int = 0,
                 keep: Optional[torch.Tensor] = None, pbest_loc: Optional[torch.Tensor] = None, loc: Optional[torch.Tensor] = None,
                 vel: Optional[torch.Tensor] = None, queries: Optional[torch.Tensor] = None):
        """dmad_pso_init: x, lower, upper (and keep) [B,1,L] or [B,L] -> (pbest_loc, loc, vel, queries), each [B*P, L], row b*P+p particle p
        of clip b: positions uniform in [lower, upper] (particle 0 = keep[b] when given), velocities uniform in +-|lower - upper|,
        loc = pbest_loc, queries = loc + x[b]; draws keyed (seed, draw0 + b*P + p, PSO_STREAM + {0, 1}).  State tensors passed in are
        written in place."""
        xw, lo, up = self._wave(x), self._wave(lower), self._wave(upper)
        B, P = xw.shape[0], int(P)
        assert lo.shape == up.shape == xw.shape, 'x, lower and upper must have one shape'
        kp = None if keep is None else self._wave(keep)
        assert kp is None or kp.shape == xw.shape, 'keep must have the shape of x'
        pbest_loc, loc, vel, queries = (self._owned(t, (B * P, self.L), name=n) for t, n in
                                        ((pbest_loc, 'pbest_loc'), (loc, 'loc'), (vel, 'vel'), (queries, 'queries')))
        check(self.lib.dmad_pso_init(self._h, _ptr(xw), _ptr(lo), _ptr(up), B, P, _ptr(kp), int(seed), int(draw0), _ptr(pbest_loc), _ptr(loc),
                                     _ptr(vel), _ptr(queries), _stream()))
        return pbest_loc, loc, vel, queries

    def pso_step(self, x: torch.Tensor, lower: torch.Tensor, upper: torch.Tensor, pbest_loc: torch.Tensor, gbest_loc: torch.Tensor, P: int,
                 w: float, c1: float, c2: float, seed: int, draw0: int, loc: torch.Tensor, vel: torch.Tensor,
                 queries: Optional[torch.Tensor] = None):
        """dmad_pso_step: vel <- w vel + c1 r1 (pbest_loc - loc) + c2 r2 (gbest_loc[b] - loc), loc <- clamp(loc + vel, lower, upper),
        queries <- loc + x[b], with r = uniform + 1e-5 keyed (seed, draw0 + b*P + p, PSO_STREAM + {2, 3}).  loc, vel (and queries) are
        updated in place and returned; gbest_loc is [B,1,L] or [B,L] in the order of x."""
        xw, lo, up, gb = self._wave(x), self._wave(lower), self._wave(upper), self._wave(gbest_loc)
        B, P = xw.shape[0], int(P)
        assert lo.shape == up.shape == gb.shape == xw.shape, 'x, lower, upper and gbest_loc must have one shape'
        rows = (B * P, self.L)
        pbest_loc, loc, vel = self._owned(pbest_loc, rows, name='pbest_loc'), self._owned(loc, rows, name='loc'), self._owned(vel, rows, name='vel')
        queries = self._owned(queries, rows, name='queries')
        check(self.lib.dmad_pso_step(self._h, _ptr(xw), _ptr(lo), _ptr(up), _ptr(pbest_loc), _ptr(gb), B, P, float(w), float(c1), float(c2),
                                     int(seed), int(draw0), _ptr(loc), _ptr(vel), _ptr(queries), _stream()))
        return loc, vel, queries

    def pso_update_best(self, loss: torch.Tensor, predict: torch.Tensor, loc: torch.Tensor, pbests: torch.Tensor, pbest_loc: torch.Tensor,
                        gbests: torch.Tensor, gbest_loc: torch.Tensor, gbest_predict: torch.Tensor, index: Optional[torch.Tensor] = None):
        """dmad_pso_update_best: loss fp32 [B,P], predict int64 [B,P], loc [B*P,L]; where loss < pbests the personal bests take loss and
        loc; then the first arg-min k of pbests[b] replaces the global best of row i = index[b] (b without index) of gbests [N],
        gbest_loc [N,L] / [N,1,L], gbest_predict int64 [N] where pbests[b][k] < gbests[i].  The five best tensors are updated in place and
        returned."""
        _on_gpu(loss)
        assert loss.dim() == 2, 'expected loss [B,P], got %s' % (tuple(loss.shape),)
        B, P = loss.shape
        loss = self._owned(_f32(loss), (B, P), name='loss')
        predict = self._owned(predict.contiguous(), (B, P), torch.int64, 'predict')
        loc, pbest_loc = self._owned(loc, (B * P, self.L), name='loc'), self._owned(pbest_loc, (B * P, self.L), name='pbest_loc')
        pbests = self._owned(pbests, (B, P), name='pbests')
        assert gbests.dim() == 1, 'expected gbests [N]'
        N = gbests.shape[0]
        gbests, gbest_predict = self._owned(gbests, (N,), name='gbests'), self._owned(gbest_predict, (N,), torch.int64, 'gbest_predict')
        assert gbest_loc.is_cuda and gbest_loc.is_contiguous() and gbest_loc.dtype == torch.float32 and gbest_loc.numel() == N * self.L, \
            'gbest_loc: expected contiguous fp32 [%d,%d]' % (N, self.L)
        if index is None:
            assert N == B, 'without index, gbests must have one row per clip'
        else:
            index = self._owned(index, (B,), torch.int64, 'index')
        check(self.lib.dmad_pso_update_best(self._h, _ptr(loss), _ptr(predict), _ptr(loc), _ptr(index), B, P, _ptr(pbests), _ptr(pbest_loc),
                                            _ptr(gbests), _ptr(gbest_loc), _ptr(gbest_predict), _stream()))
        return pbests, pbest_loc, gbests, gbest_loc, gbest_predict

    # ------------------------------------------------------------------ whole-clip real FFT pair and the Kenansville bisection
    def _fft_check(self, rc: int):
        """check() of the FFT pair: a clip_len the plan does not serve (DMAD_ERR_SHAPE) is refused with the way out"""
        try:
            check(rc)
        except DmadError as err:
            if 'the wave FFT does not serve clip_len' not in str(err):
                raise
            raise DmadError("%s; Kenansville(fft_backend='torch') (torch.fft) serves any length" % err) from None

    def wave_rfft(self, x: torch.Tensor):
        """dmad_wave_rfft: x [B,L] or [B,1,L] -> (spec [B, L/2 + 1, 2] fp32 (re, im) = torch.fft.rfft(x), maxmag [B] = max_k |spec[b][k]|).
        One workgroup per clip, exact fp32 in a fixed order; B is not limited by max_batch."""
        xw = self._wave(x)
        B = xw.shape[0]
        spec = torch.empty((B, self.L // 2 + 1, 2), device=xw.device, dtype=torch.float32)
        maxmag = torch.empty((B,), device=xw.device, dtype=torch.float32)
        self._fft_check(self.lib.dmad_wave_rfft(self._h, _ptr(xw), B, _ptr(spec), _ptr(maxmag), _stream()))
        return spec, maxmag

    def wave_irfft_threshold(self, spec: torch.Tensor, factor: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                             kept: Optional[torch.Tensor] = None):
        """dmad_wave_irfft_threshold: spec [B, L/2 + 1, 2] (as wave_rfft returns it), factor fp32 [B] or None -> (out [B,L] = irfft of spec
        with every bin |X| < factor[b] zeroed, kept int32 [B] = the surviving bins).  None: the plain inverse.  `out` / `kept` passed in
        are written in place."""
        _on_gpu(spec)
        assert spec.dim() == 3 and tuple(spec.shape[1:]) == (self.L // 2 + 1, 2), \
            'expected spec [B,%d,2], got %s' % (self.L // 2 + 1, tuple(spec.shape))
        B = spec.shape[0]
        spec = self._owned(_f32(spec), (B, self.L // 2 + 1, 2), name='spec')
        if factor is not None:
            _on_gpu(factor)
            factor = self._owned(_f32(factor), (B,), name='factor')
        out = self._owned(out, (B, self.L), name='out')
        kept = self._owned(kept, (B,), torch.int32, 'kept')
        self._fft_check(self.lib.dmad_wave_irfft_threshold(self._h, _ptr(spec), _ptr(factor), B, _ptr(out), _ptr(kept), _stream()))
        return out, kept

    def kenan_update(self, pred: torch.Tensor, label: torch.Tensor, targeted: bool, perturbed: torch.Tensor, best: torch.Tensor,
                     fmin: torch.Tensor, fmax: torch.Tensor, factor: torch.Tensor, succ: torch.Tensor):
        """dmad_kenan_update: pred, label int64 [B]; perturbed, best fp32 [B,L]; fmin, fmax, factor fp32 [B]; succ int32 [B].  Where the
        clip won (pred != label, or == when targeted): best[b] <- perturbed[b], fmax[b] <- factor[b], succ[b] <- 1; else fmin[b] <-
        factor[b]; then factor[b] <- |(fmin[b] + fmax[b]) / 2| in torch's fp32 order.  best, fmin, fmax, factor and succ are updated in
        place and returned."""
        _on_gpu(pred, label)
        assert pred.dim() == 1, 'expected pred [B], got %s' % (tuple(pred.shape),)
        B = pred.shape[0]
        pred = self._owned(pred.contiguous(), (B,), torch.int64, 'pred')
        label = self._owned(label.contiguous(), (B,), torch.int64, 'label')
        perturbed, best = self._owned(perturbed, (B, self.L), name='perturbed'), self._owned(best, (B, self.L), name='best')
        fmin, fmax, factor = (self._owned(t, (B,), name=n) for t, n in ((fmin, 'fmin'), (fmax, 'fmax'), (factor, 'factor')))
        succ = self._owned(succ, (B,), torch.int32, 'succ')
        check(self.lib.dmad_kenan_update(self._h, _ptr(pred), _ptr(label), B, int(bool(targeted)), _ptr(perturbed), _ptr(best), _ptr(fmin),
                                         _ptr(fmax), _ptr(factor), _ptr(succ), _stream()))
        return best, fmin, fmax, factor, succ

    # ------------------------------------------------------------------ baseline waveform defenses (dmad_wave_*)
    @staticmethod
    def _host_f32(a, n: Optional[int] = None):
        a = np.ascontiguousarray(_as_np(a), dtype=np.float32).reshape(-1)
        if n is not None and a.size != n:
            raise DmadError('expected %d coefficients, got %d' % (n, a.size))
        return a, a.ctypes.data_as(C.POINTER(C.c_float))

    @staticmethod
    def _fir(ker):
        """a polyphase FIR on the host -> (the array its pointer needs alive, pointer, phases, taps)"""
        k = np.ascontiguousarray(_as_np(ker), dtype=np.float32)
        phases, taps = (1, k.shape[0]) if k.ndim == 1 else k.shape
        return Engine._host_f32(k) + (int(phases), int(taps))

    def _iir(self, b, a):
        """the coefficients of an IIR filter -> (b, a on the host, their pointers, the order)"""
        bb, bp = self._host_f32(b)
        aa, ap = self._host_f32(a, bb.size)
        return bb, aa, bp, ap, bb.size - 1

    def wave_smooth(self, x: torch.Tensor, kind: int, window: int) -> torch.Tensor:
        """dmad_wave_smooth: x [B,L] or [B,1,L] -> [B,L]; kind 0 the zero-padded windowed mean (AS), 1 the median (MS)."""
        return self._mapped(self.lib.dmad_wave_smooth, self._wave(x), _N, int(kind), int(window))

    def wave_smooth_vjp(self, x: torch.Tensor, g_y: torch.Tensor, kind: int, window: int) -> torch.Tensor:
        """dmad_wave_smooth_vjp: g_x [B,L] of wave_smooth at x for the output gradient g_y (the median routes by the lowest-position rule)."""
        xw, g = self._wave(x), self._wave(g_y)
        if g.shape[0] != xw.shape[0]:
            raise DmadError('g_y has %d rows, x %d' % (g.shape[0], xw.shape[0]))
        gx = torch.empty_like(xw)
        self._passes(self.lib.dmad_wave_smooth_vjp, xw.shape[0], _per(xw), _per(g), _N, int(kind), int(window), _per(gx))
        return gx

    def wave_resample(self, x: torch.Tensor, ker, stride: int, width: int, L_out: int) -> torch.Tensor:
        """dmad_wave_resample: x [B, L_in] -> [B, L_out] through the polyphase FIR `ker` (host [phases, taps])."""
        _, kp, phases, taps = self._fir(ker)
        xw = self._rows(x, x.shape[-1])
        y = torch.empty((xw.shape[0], int(L_out)), device=xw.device, dtype=torch.float32)
        self._passes(self.lib.dmad_wave_resample, xw.shape[0], _per(xw), _N, xw.shape[1], kp, phases, taps, int(stride), int(width), int(L_out),
                     _per(y))
        return y

    def wave_resample_vjp(self, g_y: torch.Tensor, L_in: int, ker, stride: int, width: int) -> torch.Tensor:
        """dmad_wave_resample_vjp: the transposed operator, g_y [B, L_out] -> g_x [B, L_in]."""
        _, kp, phases, taps = self._fir(ker)
        g = self._rows(g_y, g_y.shape[-1], 'g_y')
        gx = torch.empty((g.shape[0], int(L_in)), device=g.device, dtype=torch.float32)
        self._passes(self.lib.dmad_wave_resample_vjp, g.shape[0], _per(g), _N, int(L_in), kp, phases, taps, int(stride), int(width), g.shape[1],
                     _per(gx))
        return gx

    def wave_iir(self, x: torch.Tensor, b, a, lo: float = -float('inf'), hi: float = float('inf')) -> torch.Tensor:
        """dmad_wave_iir: clamp(lfilter(b, a, x), lo, hi) on [B,L] rows; b, a host arrays of order + 1 <= 9 coefficients."""
        xw = self._wave(x)
        _, _, bp, ap, order = self._iir(b, a)
        return self._mapped(self.lib.dmad_wave_iir, xw, _N, bp, ap, order, float(lo), float(hi))

    def wave_iir_vjp(self, x: torch.Tensor, g_y: torch.Tensor, b, a, lo: float = -float('inf'), hi: float = float('inf'),
                     want_y: bool = False):
        """dmad_wave_iir_vjp: g_x = flip(lfilter(b, a, flip(g_y * m))), m the in-range mask of the recomputed unclamped forward.
        want_y: also return the clamped forward, bit-identical to wave_iir."""
        xw, g = self._wave(x), self._wave(g_y)
        if g.shape[0] != xw.shape[0]:
            raise DmadError('g_y has %d rows, x %d' % (g.shape[0], xw.shape[0]))
        _, _, bp, ap, order = self._iir(b, a)
        gx = torch.empty_like(xw)
        y = torch.empty_like(xw) if want_y else None
        self._passes(self.lib.dmad_wave_iir_vjp, xw.shape[0], _per(xw), _per(g), _N, bp, ap, order, float(lo), float(hi), _per(gx), _per(y))
        return (gx, y) if want_y else gx

    def defense_query_logits(self, x: torch.Tensor, repeats: int, defense: dict):
        """dmad_defense_query_logits: x [B,1,L] -> (logits [repeats*B, C], decisions int32 [repeats*B]); row r*B+b is clip b through
        defense -> mel dB -> classifier.  `defense`: dict(kind='AS'|'MS', window=w) | dict(kind='DS', down=(ker, stride, width, L_out),
        up=(ker, stride, width)) | dict(kind='IIR', b=, a=, lo=, hi=)."""
        return self._defense_query(self.lib.dmad_defense_query_logits, self.num_classes, x, repeats, defense)

    def _defense_query(self, fn, width: int, x: torch.Tensor, repeats: int, defense: dict):
        from ._lib import DmadWaveDefense
        xw = self._wave(x)
        B = xw.shape[0]
        kind = defense['kind']
        d = DmadWaveDefense(kind={'AS': 0, 'MS': 1, 'DS': 2, 'IIR': 3}[kind])
        keep = []                                   # the host arrays the struct points to
        if kind in ('AS', 'MS'):
            d.window = int(defense['window'])
        elif kind == 'DS':
            (dk, ds, dw, dl), (uk, us, uw) = defense['down'], defense['up']
            dk, uk = (np.atleast_2d(np.ascontiguousarray(_as_np(k), dtype=np.float32)) for k in (dk, uk))
            keep += [dk, uk]
            d.down_ker, d.up_ker = (k.ctypes.data_as(C.POINTER(C.c_float)) for k in (dk, uk))
            d.down_phases, d.down_taps, d.down_stride, d.down_width, d.down_len = dk.shape[0], dk.shape[1], int(ds), int(dw), int(dl)
            d.up_phases, d.up_taps, d.up_stride, d.up_width = uk.shape[0], uk.shape[1], int(us), int(uw)
        else:
            bb, aa, d.b, d.a, d.order = self._iir(defense['b'], defense['a'])
            keep += [bb, aa]
            d.lo, d.hi = float(defense['lo']), float(defense['hi'])
        logits, dec = self._logits_pair(repeats * B, width, xw.device)
        check(fn(self._h, _ptr(xw), B, int(repeats), C.byref(d), _ptr(logits), _ptr(dec), _stream()))
        del keep
        return logits, dec

    # ------------------------------------------------------------------ M5 (dmad_m5_*): waveform in, log-probabilities out
    def _m5_width(self) -> int:
        return self.m5_classes if self.has_m5 else 1        # before load_m5 the calls themselves refuse (DMAD_ERR_STATE)

    def m5_logits(self, x: torch.Tensor, want_decisions: bool = False):
        """dmad_m5_logits: x [B,1,L] or [B,L] -> log-probabilities [B, m5_classes] (and, want_decisions, their int32 arg-max).  One
        launch whatever B is: M5 has no workspace that max_batch would size, and a clip's bits do not depend on the batch (a pass of
        max_batch rows would leave most CUs idle: one workgroup per clip)."""
        xw = self._wave(x)
        B = xw.shape[0]
        out = torch.empty((B, self._m5_width()), device=xw.device, dtype=torch.float32)
        dec = torch.empty((B,), device=xw.device, dtype=torch.int32) if want_decisions else None
        check(self.lib.dmad_m5_logits(self._h, _ptr(xw), B, _ptr(out), _ptr(dec), _stream()))
        return (out, dec) if want_decisions else out

    def m5_rs_smooth_votes(self, clip: torch.Tensor, sigma: float, n: int, seed: int = 0, sample0: int = 0,
                           delta: Optional[torch.Tensor] = None, want_logits: bool = False, counts: Optional[torch.Tensor] = None):
        """dmad_m5_rs_smooth_votes: the Monte Carlo loop of RobustCertificate(M5, transform=None, denoiser=None) in one call, one
        workgroup per sample; the noisy clips exist in LDS only.  Returns (counts[int64, m5_classes] on device, log-probabilities|None),
        bit for bit what m5_logits(clip + sigma * philox_normal(seed, sample0, 0, n)) and its first maxima give."""
        clip = self._clip(clip)
        if clip.data_ptr() % 16:
            clip = clip.clone()
        if counts is None:
            counts = torch.zeros(self._m5_width(), dtype=torch.int64, device=clip.device)
        assert counts.is_cuda and counts.dtype == torch.int64 and counts.numel() == self._m5_width()
        logp = torch.empty((n, self._m5_width()), device=clip.device) if want_logits else None
        delta = self._noise_rows(delta, n)
        check(self.lib.dmad_m5_rs_smooth_votes(self._h, _ptr(clip), float(sigma), int(n), int(seed), int(sample0), _ptr(delta), _ptr(counts),
                                               _ptr(logp), _stream()))
        return counts, logp

    def m5_vjp(self, x: torch.Tensor, g: torch.Tensor, want_logits: bool = False):
        """dmad_m5_vjp: g_x [B,L] = (d logp / d x)^T g for logp = M5(x), g [B, m5_classes].  want_logits: also the log-probabilities,
        bit-identical to m5_logits(x).  The forward is recomputed inside the call; nothing is saved or reserved."""
        xw = self._wave(x)
        B = xw.shape[0]
        if not g.is_cuda or (self.has_m5 and tuple(g.shape) != (B, self.m5_classes)):
            raise DmadError('g must be a CUDA tensor [%d, %d], not %s' % (B, self.m5_classes, tuple(g.shape)))
        gl = _f32(g)
        gx = torch.empty((B, self.L), device=xw.device, dtype=torch.float32)
        lp = torch.empty((B, self._m5_width()), device=xw.device, dtype=torch.float32) if want_logits else None
        check(self.lib.dmad_m5_vjp(self._h, _ptr(xw), B, _ptr(gl), _ptr(gx), _ptr(lp), _stream()))
        return (gx, lp) if want_logits else gx

    def m5_tape(self, x: torch.Tensor, layer: int):
        """dmad_m5_tape (test hook): block `layer` (1..4) -> (pooled post-ReLU map [B,C,T] float32, decisions [B,C,T] uint8 = arg | on << 2)
        as the launch of m5_vjp produces them."""
        xw = self._wave(x)
        B = xw.shape[0]
        if layer not in (1, 2, 3, 4):
            raise DmadError('layer must be 1..4, not %r' % (layer,))
        c, t = self.m5_maps[layer - 1] if self.has_m5 else (1, 1)       # before load_m5 the call itself refuses (DMAD_ERR_STATE)
        pooled = torch.empty((B, c, t), device=xw.device, dtype=torch.float32)
        dec = torch.empty((B, c, t), device=xw.device, dtype=torch.uint8)
        check(self.lib.dmad_m5_tape(self._h, _ptr(xw), B, int(layer), _ptr(pooled), _ptr(dec), _stream()))
        return pooled, dec

    def m5_query_logits(self, x: torch.Tensor, repeats: int, sampler: int = 0, t_star: int = 0, c_a: float = 0.0, c_b: float = 0.0,
                        c_eps=None, c_div=None, c_sig=None, seed: int = 0, sample0: int = 0):
        """dmad_m5_query_logits: query_logits with M5 in the place of mel dB -> classifier; (log-probabilities [repeats*B, m5_classes],
        decisions int32 [repeats*B]); row r*B+b is clip b."""
        return self._query(self.lib.dmad_m5_query_logits, self._m5_width(), x, repeats, sampler, t_star, c_a, c_b, c_eps, c_div, c_sig, seed, sample0)

    def m5_defense_query_logits(self, x: torch.Tensor, repeats: int, defense: dict):
        """dmad_m5_defense_query_logits: defense_query_logits with M5 in the place of mel dB -> classifier (`defense` as there)."""
        return self._defense_query(self.lib.dmad_m5_defense_query_logits, self._m5_width(), x, repeats, defense)

    # ------------------------------------------------------------------ KWS (dmad_kws_*): dB mel spectrogram in, log-probabilities out
    @staticmethod
    def _kws_spec(x: torch.Tensor) -> torch.Tensor:
        """[B,1,32,T] or [B,32,T] -> contiguous fp32 [B,32,T]; T is an argument of every call, and the library checks it"""
        _on_gpu(x)
        x = x.detach()
        if x.dim() == 4:
            assert x.shape[1] == 1, 'expected [B,1,%d,T]' % KWS_BINS
            x = x[:, 0]
        assert x.dim() == 3 and x.shape[1] == KWS_BINS, 'expected [B,%d,T], got %s' % (KWS_BINS, tuple(x.shape))
        return x.contiguous().float()

    def kws_logits(self, spec: torch.Tensor, want_decisions: bool = False):
        """dmad_kws_logits: spec [B,1,32,T] or [B,32,T] -> log-probabilities [B,4] (and, want_decisions, their int32 arg-max).  One launch
        whatever B is, like m5_logits: no workspace that max_batch would size, and a row's bits do not depend on the batch."""
        xs = self._kws_spec(spec)
        B, T = xs.shape[0], xs.shape[2]
        out = torch.empty((B, KWS_CLASSES), device=xs.device, dtype=torch.float32)
        dec = torch.empty((B,), device=xs.device, dtype=torch.int32) if want_decisions else None
        check(self.lib.dmad_kws_logits(self._h, _ptr(xs), B, T, _ptr(out), _ptr(dec), _stream()))
        return (out, dec) if want_decisions else out

    def kws_vjp(self, spec: torch.Tensor, g: torch.Tensor, want_logits: bool = False):
        """dmad_kws_vjp: g_spec [B,32,T] = (d logp / d spec)^T g for logp = KWSModel(spec), g [B,4]; exact zeros at the frames no GRU
        step reads.  want_logits: also the log-probabilities, bit-identical to kws_logits(spec).  The forward is recomputed inside the
        call; nothing is saved or reserved."""
        xs = self._kws_spec(spec)
        B, T = xs.shape[0], xs.shape[2]
        if not g.is_cuda or tuple(g.shape) != (B, KWS_CLASSES):
            raise DmadError('g must be a CUDA tensor [%d, %d], not %s' % (B, KWS_CLASSES, tuple(g.shape)))
        gl = _f32(g)
        gs = torch.empty_like(xs)
        lp = torch.empty((B, KWS_CLASSES), device=xs.device, dtype=torch.float32) if want_logits else None
        check(self.lib.dmad_kws_vjp(self._h, _ptr(xs), B, T, _ptr(gl), _ptr(gs), _ptr(lp), _stream()))
        return (gs, lp) if want_logits else gs

    def kws_tape(self, spec: torch.Tensor, stage: int) -> torch.Tensor:
        """dmad_kws_tape (test hook), as the launch of kws_vjp produces them: stage 0 the sepconv output [B,T2,64], 1 / 2 the output of GRU
        layer 0 / 1 [B,T2,128] (forward direction first), 3 the attention scores [B,T2]."""
        xs = self._kws_spec(spec)
        B, T = xs.shape[0], xs.shape[2]
        if stage not in (0, 1, 2, 3):
            raise DmadError('stage must be 0..3, not %r' % (stage,))
        t2 = max(kws_steps(T), 1)              # a T the library refuses still needs a buffer to pass
        out = torch.empty((B, t2) + ((64,), (128,), (128,), ())[stage], device=xs.device, dtype=torch.float32)
        check(self.lib.dmad_kws_tape(self._h, _ptr(xs), B, T, int(stage), _ptr(out), _stream()))
        return out

    # ------------------------------------------------------------------ the KWS mel front-end (dmad_kws_mel_*, dmad_kws_wave_*): any clip length
    @staticmethod
    def _kws_wave(x: torch.Tensor) -> torch.Tensor:
        """[B,1,L] or [B,L] -> contiguous fp32 [B,L]; L is an argument of every call, and the library checks it"""
        _on_gpu(x)
        x = x.detach()
        if x.dim() == 3:
            assert x.shape[1] == 1, 'expected [B,1,L]'
            x = x[:, 0]
        assert x.dim() == 2, 'expected [B,L], got %s' % (tuple(x.shape),)
        return x.contiguous().float()

    def _kws_mel(self, fn, x):
        xw = self._kws_wave(x)
        B, L = xw.shape
        out = torch.empty((B, KWS_BINS, kws_frames(L)), device=xw.device, dtype=torch.float32)
        check(fn(self._h, _ptr(xw), B, L, _ptr(out), _stream()))
        return out

    def kws_mel_power(self, x: torch.Tensor) -> torch.Tensor:
        """dmad_kws_mel_power: x [B,1,L] or [B,L] -> mel power [B,32,T], T = 1 + L // 200 (torchaudio MelSpectrogram(16000, n_mels=32)).
        One launch whatever B and L are."""
        return self._kws_mel(self.lib.dmad_kws_mel_power, x)

    def kws_mel_db(self, x: torch.Tensor) -> torch.Tensor:
        """dmad_kws_mel_db: kws_mel_power followed by AmplitudeToDB('power'), in the same launch."""
        return self._kws_mel(self.lib.dmad_kws_mel_db, x)

    def kws_mel_db_vjp(self, x: torch.Tensor, g_spec: torch.Tensor, want_spec: bool = False):
        """dmad_kws_mel_db_vjp: g_x [B,L] = (d kws_mel_db / d x)^T g_spec for g_spec [B,32,T] (or [B,1,32,T]).  want_spec: also the dB
        spectrogram, bit-identical to kws_mel_db(x).  The forward is recomputed inside the one launch; nothing is saved or reserved."""
        xw = self._kws_wave(x)
        B, L = xw.shape
        T = kws_frames(L)
        if not g_spec.is_cuda or g_spec.numel() != B * KWS_BINS * T or g_spec.shape[-1] != T:
            raise DmadError('g_spec must be a CUDA tensor [%d, %d, %d], not %s' % (B, KWS_BINS, T, tuple(g_spec.shape)))
        gs = _f32(g_spec)
        gx = torch.empty_like(xw)
        spec = torch.empty((B, KWS_BINS, T), device=xw.device, dtype=torch.float32) if want_spec else None
        check(self.lib.dmad_kws_mel_db_vjp(self._h, _ptr(xw), B, L, _ptr(gs), _ptr(gx), _ptr(spec), _stream()))
        return (gx, spec) if want_spec else gx

    def kws_wave_logits(self, x: torch.Tensor, want_decisions: bool = False):
        """dmad_kws_wave_logits: x [B,1,L] or [B,L] -> log-probabilities [B,4] of KWSModel behind its mel front-end, bit-identical to
        kws_logits(kws_mel_db(x)); only the spectrogram frames the model reads are computed.  One library call whatever B is."""
        xw = self._kws_wave(x)
        B, L = xw.shape
        out = torch.empty((B, KWS_CLASSES), device=xw.device, dtype=torch.float32)
        dec = torch.empty((B,), device=xw.device, dtype=torch.int32) if want_decisions else None
        check(self.lib.dmad_kws_wave_logits(self._h, _ptr(xw), B, L, _ptr(out), _ptr(dec), _stream()))
        return (out, dec) if want_decisions else out

    def kws_wave_vjp(self, x: torch.Tensor, g: torch.Tensor, want_logits: bool = False):
        """dmad_kws_wave_vjp: g_x [B,L] = (d logp / d x)^T g for logp = KWSModel(kws_mel_db(x)), g [B,4]; bit-identical to
        kws_mel_db_vjp(x, kws_vjp(kws_mel_db(x), g)).  want_logits: also the log-probabilities, bit-identical to kws_wave_logits(x)."""
        xw = self._kws_wave(x)
        B, L = xw.shape
        if not g.is_cuda or tuple(g.shape) != (B, KWS_CLASSES):
            raise DmadError('g must be a CUDA tensor [%d, %d], not %s' % (B, KWS_CLASSES, tuple(g.shape)))
        gl = _f32(g)
        gx = torch.empty_like(xw)
        lp = torch.empty((B, KWS_CLASSES), device=xw.device, dtype=torch.float32) if want_logits else None
        check(self.lib.dmad_kws_wave_vjp(self._h, _ptr(xw), B, L, _ptr(gl), _ptr(gx), _ptr(lp), _stream()))
        return (gx, lp) if want_logits else gx

    def kws_query_logits(self, x: torch.Tensor, repeats: int, sampler: int = 0, t_star: int = 0, c_a: float = 0.0, c_b: float = 0.0,
                         c_eps=None, c_div=None, c_sig=None, seed: int = 0, sample0: int = 0):
        """dmad_kws_query_logits: query_logits with mel dB -> KWSModel in the place of mel dB -> classifier; x [B,1,clip_len] ->
        (log-probabilities [repeats*B, 4], decisions int32 [repeats*B]); row r*B+b is clip b."""
        return self._query(self.lib.dmad_kws_query_logits, KWS_CLASSES, x, repeats, sampler, t_star, c_a, c_b, c_eps, c_div, c_sig, seed, sample0)

    def kws_defense_query_logits(self, x: torch.Tensor, repeats: int, defense: dict):
        """dmad_kws_defense_query_logits: defense_query_logits with mel dB -> KWSModel behind the defense (`defense` as there)."""
        return self._defense_query(self.lib.dmad_kws_defense_query_logits, KWS_CLASSES, x, repeats, defense)

    # ------------------------------------------------------------------ Philox draws, timing and profiling hooks
    def _philox(self, fn, seed, sample0, stream, B):
        out = torch.empty((B, self.L), dtype=torch.float32, device=self.device)
        check(fn(self._h, int(seed), int(sample0), int(stream), int(B), _ptr(out), _stream()))
        return out

    def philox_uniform(self, seed: int, sample0: int, stream: int, B: int) -> torch.Tensor:
        """dmad_philox_uniform: [B, L], row b the uniforms ((word >> 8) + 0.5) * 2^-24 of key (seed, sample0 + b, stream)."""
        return self._philox(self.lib.dmad_philox_uniform, seed, sample0, stream, B)

    def philox_normal(self, seed: int, sample0: int, stream: int, B: int, length: Optional[int] = None) -> torch.Tensor:
        """[B, L] normals of key (seed, sample0 + b, stream); length: [B, length], the first `length` values of those rows
        (dmad_philox_normal_len, 1 <= length <= L)."""
        if length is None:
            return self._philox(self.lib.dmad_philox_normal, seed, sample0, stream, B)
        out = torch.empty((B, int(length)), dtype=torch.float32, device=self.device)
        check(self.lib.dmad_philox_normal_len(self._h, int(seed), int(sample0), int(stream), int(B), int(length), _ptr(out), _stream()))
        return out

    def philox_raw(self, seed: int, sample: int, stream: int, nblocks: int) -> torch.Tensor:
        out = torch.empty(nblocks * 4, dtype=torch.int32, device=self.device)
        check(self.lib.dmad_philox_raw(self._h, int(seed), int(sample), int(stream), int(nblocks), _ptr(out), _stream()))
        return out

    def time_layer(self, layer: int, B: int, iters: int) -> float:
        ms = C.c_float(0)
        check(self.lib.dmad_time_layer(self._h, int(layer), int(B), int(iters), C.byref(ms), _stream()))
        return float(ms.value)

    def profile_layers(self, max_launches: int):
        check(self.lib.dmad_profile_layers(self._h, int(max_launches)))

    def _profile(self, fn):
        ms, n = C.c_float(0), C.c_int32(0)
        check(fn(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def profile_read(self):
        """-> (summed ms, launches) of the bracketed wn_layer_bf16 launches."""
        return self._profile(self.lib.dmad_profile_read)

    def profile_read_final(self):
        """-> (summed ms, launches) of the bracketed wn_final launches; call before profile_read()."""
        return self._profile(self.lib.dmad_profile_read_final)

    def device_bytes(self) -> int:
        return int(self.lib.dmad_device_bytes(self._h))


# ---------------------------------------------------------------------- standalone op hooks (no engine: test / measurement)
def _op(export: str, *args):
    """one call of an engine-less export on the current stream"""
    check(getattr(_lib.load(), export)(*args, _stream()))


def conv_h16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, stride: int = 1, groups: int = 1, relu: bool = False,
             res: Optional[torch.Tensor] = None, x2: Optional[torch.Tensor] = None, want32: bool = True, want16: bool = True):
    """dmad_conv_h16 — the f16 conv-GEMM family as a standalone op (test hook).  x: f16 NHWC [B,H,H,Cx] (CUDA), x2: optional second
    map [B,H,H,C2] whose channels follow x's (dense convs only); w: f16 [groups, taps, M, K] (taps 9 or 1, K per group = (Cx + C2) /
    groups); bias fp32 [groups*M]; res: optional f16 [B,Ho,Ho,groups*M].  Returns (out32 | None, out16 | None), NHWC."""
    assert x.is_cuda and x.dtype == torch.float16 and w.is_cuda and w.dtype == torch.float16 and x.dim() == 4 and w.dim() == 4
    x, w = x.contiguous(), w.contiguous()
    B, H, W_, cx = x.shape
    assert H == W_
    g_, taps, M, K = w.shape
    assert g_ == groups and taps in (1, 9)
    ksplit = 0
    if x2 is not None:
        assert groups == 1 and x2.dtype == torch.float16 and x2.shape[:3] == x.shape[:3]
        x2 = x2.contiguous()
        ksplit = cx
        assert cx + x2.shape[3] == K
    else:
        assert cx == groups * K
    Ho = (H - 1) // stride + 1
    out32 = torch.empty((B, Ho, Ho, groups * M), device=x.device, dtype=torch.float32) if want32 else None
    out16 = torch.empty((B, Ho, Ho, groups * M), device=x.device, dtype=torch.float16) if want16 else None
    if res is not None:
        assert res.dtype == torch.float16 and tuple(res.shape) == (B, Ho, Ho, groups * M)
        res = res.contiguous()
    _op('dmad_conv_h16', _ptr(x), _ptr(x2), int(ksplit), _ptr(w), _ptr(_f32(bias)), _ptr(res), B, H, M, K, taps, int(stride), int(groups),
        1 if relu else 0, _ptr(out32), _ptr(out16))
    return out32, out16


def conv_h16_up2(x_half: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, want_stats: bool = False):
    """dmad_conv_h16_up2 — nearest x2 upsampling + 3x3 conv in one launch (test hook of GemmH16Args::up2).  x_half: f16 NHWC
    [B,H/2,H/2,K]; w: f16 [1,9,M,K]; res: optional f16 [B,H,H,M].  Returns (out32, out16, stats | None); raises DmadError when the shape
    is not served by the fusing form."""
    assert x_half.is_cuda and x_half.dtype == torch.float16 and w.dtype == torch.float16 and w.shape[0] == 1 and w.shape[1] == 9
    x_half, w = x_half.contiguous(), w.contiguous()
    B, Hh, _, K = x_half.shape
    M, H = w.shape[2], 2 * Hh
    assert w.shape[3] == K
    out32 = torch.empty((B, H, H, M), device=x_half.device, dtype=torch.float32)
    out16 = torch.empty((B, H, H, M), device=x_half.device, dtype=torch.float16)
    stats = torch.zeros((B * H * H // 64, M // 4, 2), device=x_half.device, dtype=torch.float32) if want_stats else None
    if res is not None:
        assert res.dtype == torch.float16 and tuple(res.shape) == (B, H, H, M)
        res = res.contiguous()
    _op('dmad_conv_h16_up2', _ptr(x_half), _ptr(w), _ptr(_f32(bias)), _ptr(res), B, H, M, K, _ptr(out32), _ptr(out16), _ptr(stats))
    return out32, out16, stats


def split_f16(x: torch.Tensor) -> torch.Tensor:
    """dmad_split_f16: the split-f16 storage form (hi / lo f16 pairs in the bytes of the floats) of an fp32 CUDA tensor whose last dimension is a
    multiple of 4; returned as a float32 tensor of the same shape (its bits are NOT floats)."""
    assert x.is_cuda and x.dtype == torch.float32 and x.shape[-1] % 4 == 0
    x = x.contiguous()
    y = torch.empty_like(x)
    _op('dmad_split_f16', _ptr(x), x.numel(), _ptr(y))
    return y


def conv_x3(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, stride: int = 1, relu: bool = False,
            res: Optional[torch.Tensor] = None, x2: Optional[torch.Tensor] = None, out_split: bool = False, groups: int = 1,
            res_split: bool = False) -> torch.Tensor:
    """dmad_conv_x3 — the split-f16 conv GEMM as a standalone op (test hook).  x: fp32 NHWC [B,H,H,Cx], x2: optional second map whose
    channels follow x's (dense only); w: fp32 [taps, M, K] (dense) or [groups, taps, M, K]; bias fp32 [groups*M]; res fp32
    [B,Ho,Ho,groups*M] (res_split: handed to the kernel in the split format).  Operands are converted with split_f16 here."""
    assert x.is_cuda and x.dtype == torch.float32 and w.is_cuda and w.dtype == torch.float32 and x.dim() == 4 and w.dim() in (3, 4)
    if w.dim() == 3:
        w = w[None]
    B, H, W_, cx = x.shape
    assert H == W_ and w.shape[0] == groups
    _, taps, M, K = w.shape
    xs, ws = split_f16(x), split_f16(w)
    x2s, ksplit = None, 0
    if x2 is not None:
        assert groups == 1 and x2.shape[:3] == x.shape[:3] and cx + x2.shape[3] == K
        x2s, ksplit = split_f16(x2), cx
    else:
        assert cx == groups * K
    Ho = (H - 1) // stride + 1
    out = torch.empty((B, Ho, Ho, groups * M), device=x.device, dtype=torch.float32)
    if res is not None:
        assert tuple(res.shape) == (B, Ho, Ho, groups * M) and res.dtype == torch.float32
        res = split_f16(res) if res_split else res.contiguous()
    _op('dmad_conv_x3', _ptr(xs), _ptr(x2s), int(ksplit), _ptr(ws), _ptr(_f32(bias)), _ptr(res), B, H, M, K, taps, int(stride), int(groups),
        1 if relu else 0, 1 if out_split else 0, 1 if res_split else 0, _ptr(out))
    return out


def conv_h16_stats(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, stride: int = 1, res: Optional[torch.Tensor] = None):
    """dmad_conv_h16_stats: dense f16 conv (x [B,H,H,K] f16, w [1,taps,M,K] f16) -> (out16 [B,Ho,Ho,M] f16, stats [B*Ho*Ho/blk, M/4, 2] fp32):
    the GroupNorm statistics the producing GEMM's epilogue leaves for groupnorm16_apply (blk = 64 pixels, 16 on 4x4 maps)."""
    assert x.is_cuda and x.dtype == torch.float16 and w.dtype == torch.float16 and w.shape[0] == 1
    x, w = x.contiguous(), w.contiguous()
    B, H, _, K = x.shape
    _, taps, M, K2 = w.shape
    assert K2 == K
    Ho = (H - 1) // stride + 1
    blk = 64 if Ho * Ho >= 64 else 16
    out16 = torch.empty((B, Ho, Ho, M), device=x.device, dtype=torch.float16)
    stats = torch.zeros((B * Ho * Ho // blk, M // 4, 2), device=x.device, dtype=torch.float32)
    if res is not None:
        res = res.contiguous()
    _op('dmad_conv_h16_stats', _ptr(x), _ptr(w), _ptr(_f32(bias)), _ptr(res), B, H, M, K, taps, int(stride), _ptr(out16), _ptr(stats))
    return out16, stats


def groupnorm16_apply(x: torch.Tensor, st: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, silu: bool = True, ss: Optional[torch.Tensor] = None,
                      x2: Optional[torch.Tensor] = None, st2: Optional[torch.Tensor] = None, out32: bool = False):
    """dmad_groupnorm16_apply: one-pass GroupNorm32 (+ scale-shift, + SiLU) of the f16 map x [B,HW,c1] (| x2 [B,HW,C-c1]) from the
    statistics slabs of conv_h16_stats.  Returns y [B,HW,C] (f16, or fp32 with out32)."""
    x, st = x.contiguous(), st.contiguous()
    B, HW, c1 = x.shape
    C = c1 + (x2.shape[2] if x2 is not None else 0)
    y = torch.empty((B, HW, C), device=x.device, dtype=torch.float32 if out32 else torch.float16)
    if x2 is not None:
        x2, st2 = x2.contiguous(), st2.contiguous()
    _op('dmad_groupnorm16_apply', _ptr(x), _ptr(st), _ptr(x2), _ptr(st2), int(c1 if x2 is not None else 0), _ptr(_f32(gamma)), _ptr(_f32(beta)),
        _ptr(_f32(ss)), 1 if silu else 0, B, HW, C, None if out32 else _ptr(y), _ptr(y) if out32 else None)
    return y


def groupnorm16(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, silu: bool = True, ss: Optional[torch.Tensor] = None,
                x2: Optional[torch.Tensor] = None, out32: bool = False) -> torch.Tensor:
    """dmad_groupnorm16: the two-pass GroupNorm32 (+ scale-shift, + SiLU) of the f16 map x [B,HW,c1] (| x2 [B,HW,C-c1]) — the form the 16-bit
    tier falls back to without a statistics slab.  Returns y [B,HW,C] (f16, or fp32 with out32) (test hook)."""
    assert x.is_cuda and x.dtype == torch.float16 and x.dim() == 3 and (x2 is None or x2.dtype == torch.float16)
    x, x2 = x.contiguous(), (None if x2 is None else x2.contiguous())
    B, HW, c1 = x.shape
    C = c1 + (x2.shape[2] if x2 is not None else 0)
    y = torch.empty((B, HW, C), device=x.device, dtype=torch.float32 if out32 else torch.float16)
    _op('dmad_groupnorm16', _ptr(x), _ptr(x2), int(c1 if x2 is not None else 0), _ptr(_f32(gamma)), _ptr(_f32(beta)), _ptr(_f32(ss)),
        1 if silu else 0, B, HW, C, None if out32 else _ptr(y), _ptr(y) if out32 else None)
    return y


def qkv_attention_h16(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """dmad_qkv_attention_h16: qkv f16 [B,T,heads*192] (head-major q | k | v) -> out f16 [B,T,heads*64] (test hook)."""
    assert qkv.is_cuda and qkv.dtype == torch.float16 and qkv.dim() == 3 and qkv.shape[2] == heads * 192
    qkv = qkv.contiguous()
    B, T, _ = qkv.shape
    out = torch.empty((B, T, heads * 64), device=qkv.device, dtype=torch.float16)
    _op('dmad_qkv_attention_h16', _ptr(qkv), B, T, int(heads), _ptr(out))
    return out


def conv1ch_3x3(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, want32: bool = True, want16: bool = True, want_stats: bool = False):
    """dmad_conv1ch_3x3: the UNet's first layer, x fp32 [B,32,32], w [Cout,9] (or [Cout,3,3]), bias [Cout] -> (out32 | None, out16 | None,
    stats | None): [B,1024,Cout] fp32 / f16 and the GroupNorm statistics slab [B*16, Cout/4, 2] of the f16-rounded outputs (test hook)."""
    x, w, bias = _f32(x), _f32(w), _f32(bias)
    assert x.is_cuda and x.dim() == 3 and tuple(x.shape[1:]) == (32, 32)
    B, Cout = x.shape[0], w.shape[0]
    assert w.numel() == Cout * 9 and bias.numel() == Cout
    out32 = torch.empty((B, 1024, Cout), device=x.device, dtype=torch.float32) if want32 else None
    out16 = torch.empty((B, 1024, Cout), device=x.device, dtype=torch.float16) if want16 else None
    stats = torch.full((B * 16, max(Cout // 4, 1), 2), float('nan'), device=x.device, dtype=torch.float32) if want_stats else None
    _op('dmad_conv1ch_3x3', _ptr(x), _ptr(w), _ptr(bias), B, Cout, _ptr(out32), _ptr(out16), _ptr(stats))
    return out32, out16, stats


def conv3x3_c128_to1(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, g_in: Optional[torch.Tensor] = None, alpha: float = 1.0,
                     gamma: float = 0.0) -> torch.Tensor:
    """dmad_conv3x3_c128_to1 / _h16: the UNet's last layer, x [B,1024,128] (fp32, or f16: the 16-bit tier's MFMA form), w fp32 [9,128]
    (tap-major), bias [1] -> out fp32 [B,1024]; with g_in [B,1024] (fp32 form only): alpha * g_in - gamma * conv (test hook)."""
    assert x.is_cuda and x.dim() == 3 and tuple(x.shape[1:]) == (1024, 128) and x.dtype in (torch.float32, torch.float16)
    x, w, bias = x.contiguous(), _f32(w), _f32(bias)
    assert w.numel() == 9 * 128 and bias.numel() == 1
    B = x.shape[0]
    out = torch.empty((B, 1024), device=x.device, dtype=torch.float32)
    if x.dtype == torch.float16:
        assert g_in is None
        _op('dmad_conv3x3_c128_to1_h16', _ptr(x), _ptr(w), _ptr(bias), B, _ptr(out))
    else:
        g_in = _f32(g_in)
        assert g_in is None or tuple(g_in.shape) == (B, 1024)
        _op('dmad_conv3x3_c128_to1', _ptr(x), _ptr(w), _ptr(bias), B, _ptr(g_in), float(alpha), float(gamma), _ptr(out))
    return out


def upsample2x(x: torch.Tensor) -> torch.Tensor:
    """dmad_upsample2x: nearest-neighbour x2 of an NHWC map x [B,H,H,C] (fp32 or f16) -> [B,2H,2H,C] (test hook)."""
    assert x.is_cuda and x.dim() == 4 and x.shape[1] == x.shape[2] and x.dtype in (torch.float32, torch.float16)
    x = x.contiguous()
    B, H, _, Cn = x.shape
    out = torch.empty((B, 2 * H, 2 * H, Cn), device=x.device, dtype=x.dtype)
    _op('dmad_upsample2x', _ptr(x), B, H, Cn, 1 if x.dtype == torch.float16 else 0, _ptr(out))
    return out


def conv_f32(x: torch.Tensor, w: torch.Tensor, shift: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None, stride: int = 1,
             groups: int = 1, relu: bool = False, res: Optional[torch.Tensor] = None, x2: Optional[torch.Tensor] = None,
             slab: Optional[torch.Tensor] = None, n_ref: int = 0):
    """dmad_conv_f32 — the exact-fp32 conv GEMM as a standalone op (test hook).  x: fp32 NHWC [B,H,H,Cx] (x2: optional second map whose
    channels follow x's), or [B,K] rows (the plain GEMM of the Linear layers); w fp32 [groups, taps, M, K] (or [taps, M, K]); scale /
    shift [groups*M]; res like the output; slab: optional fp32 split-K workspace, n_ref the row count the split count is derived from.
    Returns (out, choice) with choice = dict(bm, narrow, two, splits): what the launcher chose."""
    assert x.is_cuda and x.dtype == torch.float32 and w.is_cuda and w.dtype == torch.float32 and x.dim() in (2, 4) and w.dim() in (3, 4)
    if w.dim() == 3:
        w = w[None]
    x, w = x.contiguous(), w.contiguous()
    _, taps, M, K = w.shape
    assert w.shape[0] == groups
    x2c, ksplit = None, 0
    if x.dim() == 2:
        B, H = x.shape[0], 0
        assert x.shape[1] == K and x2 is None
        oshape = (B, M)
    else:
        B, H, W_, cx = x.shape
        assert H == W_
        if x2 is not None:
            assert x2.shape[:3] == x.shape[:3] and cx + x2.shape[3] == K
            x2c, ksplit = x2.contiguous(), cx
        else:
            assert cx == groups * K
        Ho = (H - 1) // stride + 1
        oshape = (B, Ho, Ho, groups * M)
    out = torch.empty(oshape, device=x.device, dtype=torch.float32)
    scale, shift, res = _f32(scale), _f32(shift), _f32(res)
    if res is not None:
        assert tuple(res.shape) == oshape
    choice = (C.c_int32 * 4)()
    _op('dmad_conv_f32', _ptr(x), _ptr(x2c), int(ksplit), _ptr(w), _ptr(scale), _ptr(shift), _ptr(res), B, H, M, K, taps, int(stride),
        int(groups), 1 if relu else 0, _ptr(slab), slab.numel() if slab is not None else 0, int(n_ref), _ptr(out), choice)
    return out, dict(bm=choice[0], narrow=choice[1], two=choice[2], splits=choice[3])


def conv_f32_vjp(g_y: torch.Tensor, w: torch.Tensor, H: int, form: int = 0, stride: int = 1, groups: int = 1,
                 scale: Optional[torch.Tensor] = None, mask_y: Optional[torch.Tensor] = None, acc: Optional[torch.Tensor] = None, ldt: int = 0):
    """dmad_conv_f32_vjp — the data gradient of an NHWC conv (test hook; forms of include/dmad.h: 0 UNet conv, 1 UNet Upsample, 2
    ResNeXt29, 3 VGG19_bn's dense 3x3 with its BN scale, 4 WideResNet's dense 3x3 / 1x1 at stride 1 or 2 with an optional scale).  g_y fp32 [B,Ho,Ho,groups*M] (ldt channels with a padded 1x1 image), w [groups, taps, M, K] in the forward layout, H the
    forward conv's input resolution.  Returns (g_x, wT, gm | None, work | None): the gradient, the packed weight image as the pack kernel
    wrote it, the masked gradient, and the dilated / pre-sum work map."""
    assert g_y.is_cuda and g_y.dtype == torch.float32 and w.dtype == torch.float32 and g_y.dim() == 4 and w.dim() == 4
    g_y, w = g_y.contiguous(), w.contiguous()
    _, taps, M, K = w.shape
    assert w.shape[0] == groups
    B, dev = g_y.shape[0], g_y.device
    Ho = 2 * H if form == 1 else (H - 1) // stride + 1
    kp = ldt if (form == 2 and taps == 1 and ldt) else M
    assert tuple(g_y.shape) == (B, Ho, Ho, groups * kp), (tuple(g_y.shape), (B, Ho, Ho, groups * kp))
    if form == 2 and taps == 9:
        wT = torch.full((groups, 9, K, M), float('nan'), device=dev)
    elif form == 2:
        wT = torch.full((K, kp), float('nan'), device=dev)
    else:
        wT = torch.full((taps, K, M), float('nan'), device=dev)
    g_x = torch.empty((B, H, H, groups * K), device=dev, dtype=torch.float32)
    gm = torch.empty_like(g_y) if mask_y is not None else None
    work = None
    if form == 1:
        work = torch.empty((B, 2 * H, 2 * H, K), device=dev, dtype=torch.float32)
    elif stride == 2:
        work = torch.empty((B, H, H, groups * M) if taps == 9 else (B, Ho, Ho, K), device=dev, dtype=torch.float32)
    scale, mask_y, acc = _f32(scale), _f32(mask_y), _f32(acc)
    if acc is not None:
        assert tuple(acc.shape) == tuple(g_x.shape)
    if mask_y is not None:
        assert tuple(mask_y.shape) == tuple(g_y.shape)
    _op('dmad_conv_f32_vjp', _ptr(g_y), _ptr(w), _ptr(scale), _ptr(mask_y), _ptr(acc), B, int(H), M, K, taps, int(stride), int(groups),
        int(form), int(ldt), _ptr(wT), _ptr(gm), _ptr(work), _ptr(g_x))
    return g_x, wT, gm, work


def groupnorm_f32(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, silu: bool = False, ss: Optional[torch.Tensor] = None,
                  x2: Optional[torch.Tensor] = None, split: bool = False) -> torch.Tensor:
    """dmad_groupnorm_f32: GroupNorm32 (+ scale-shift, + SiLU) of the fp32 map x [B,HW,c1] (| x2 [B,HW,C-c1]) -> y [B,HW,C] (test hook).
    split: y in the split-f16 storage form (as split_f16 returns it: its bits are NOT floats)."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3
    x, x2 = x.contiguous(), (None if x2 is None else x2.contiguous())
    B, HW, c1 = x.shape
    Cn = c1 + (x2.shape[2] if x2 is not None else 0)
    y = torch.empty((B, HW, Cn), device=x.device, dtype=torch.float32)
    _op('dmad_groupnorm_f32', _ptr(x), _ptr(x2), int(c1), _ptr(_f32(gamma)), _ptr(_f32(beta)), _ptr(_f32(ss)), 1 if silu else 0, B, HW, Cn,
        1 if split else 0, _ptr(y))
    return y


def groupnorm_bwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, gy: torch.Tensor, silu: bool = False,
                  ss: Optional[torch.Tensor] = None, x2: Optional[torch.Tensor] = None, add: Optional[torch.Tensor] = None,
                  add2: Optional[torch.Tensor] = None):
    """dmad_groupnorm_bwd: the gradient of groupnorm_f32 with respect to its input -> (gx [B,HW,c1], gx2 [B,HW,C-c1] | None), add / add2
    ([B,HW,C]) summed in (test hook)."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3
    x, x2, gy = x.contiguous(), (None if x2 is None else x2.contiguous()), gy.contiguous()
    B, HW, c1 = x.shape
    Cn = c1 + (x2.shape[2] if x2 is not None else 0)
    assert tuple(gy.shape) == (B, HW, Cn)
    gx = torch.empty_like(x)
    gx2 = torch.empty_like(x2) if x2 is not None else None
    gamma, beta, ss, add, add2 = _f32(gamma), _f32(beta), _f32(ss), _f32(add), _f32(add2)
    _op('dmad_groupnorm_bwd', _ptr(x), _ptr(x2), int(c1), _ptr(gamma), _ptr(beta), _ptr(ss), 1 if silu else 0, _ptr(gy), _ptr(add),
        _ptr(add2), B, HW, Cn, _ptr(gx), _ptr(gx2))
    return gx, gx2


def qkv_attention_f32(qkv: torch.Tensor, heads: int, split: bool = False) -> torch.Tensor:
    """dmad_qkv_attention_f32: qkv fp32 [B,T,heads*192] (head-major q | k | v) -> out [B,T,heads*64] (test hook).  split: out in the
    split-f16 storage form (as split_f16 returns it: its bits are NOT floats)."""
    assert qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 3 and qkv.shape[2] == heads * 192
    qkv = qkv.contiguous()
    B, T, _ = qkv.shape
    out = torch.empty((B, T, heads * 64), device=qkv.device, dtype=torch.float32)
    _op('dmad_qkv_attention_f32', _ptr(qkv), B, T, int(heads), 1 if split else 0, _ptr(out))
    return out


def qkv_attention_bwd(qkv: torch.Tensor, go: torch.Tensor, heads: int) -> torch.Tensor:
    """dmad_qkv_attention_bwd: the gradient of qkv_attention_f32 -> gqkv [B,T,heads*192] (dq | dk | dv per head) (test hook)."""
    assert qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 3 and qkv.shape[2] == heads * 192
    qkv, go = qkv.contiguous(), go.contiguous()
    B, T, _ = qkv.shape
    assert tuple(go.shape) == (B, T, heads * 64) and go.dtype == torch.float32
    gqkv = torch.empty_like(qkv)
    _op('dmad_qkv_attention_bwd', _ptr(qkv), _ptr(go), B, T, int(heads), _ptr(gqkv))
    return gqkv


def rx_head_bwd(g_logits: torch.Tensor, W: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """dmad_rx_head_bwd: g_logits [B,ncls], W [ncls,C], y [B,HW,C] -> gz [B,HW,C] (FC, average pool and the last ReLU backward) (test hook)."""
    g_logits, W, y = _f32(g_logits), _f32(W), _f32(y)
    B, HW, Cn = y.shape
    assert tuple(g_logits.shape) == (B, W.shape[0]) and W.shape[1] == Cn and y.is_cuda
    gz = torch.empty_like(y)
    _op('dmad_rx_head_bwd', _ptr(g_logits), _ptr(W), _ptr(y), B, int(W.shape[0]), HW, Cn, _ptr(gz))
    return gz


def vgg_pool_relu_bwd(g: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """dmad_vgg_pool_relu_bwd: g [B,H/2,H/2,C], y [B,H,H,C] (the saved post-ReLU map) -> gpre [B,H,H,C] (2x2 max-pool and the ReLU in front
    of it, backward) (test hook)."""
    g, y = _f32(g), _f32(y)
    B, H, _, Cn = y.shape
    assert y.is_cuda and y.shape[2] == H and tuple(g.shape) == (B, H // 2, H // 2, Cn)
    gpre = torch.empty_like(y)
    _op('dmad_vgg_pool_relu_bwd', _ptr(g), _ptr(y), B, H, Cn, _ptr(gpre))
    return gpre


def wrn_preact(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """dmad_wrn_preact: x [..., C] (NHWC), scale / shift [C] -> max(scale * x + shift, 0) (WideResNet's pre-activation) (test hook)."""
    x, scale, shift = _f32(x), _f32(scale), _f32(shift)
    Cn = x.shape[-1]
    assert x.is_cuda and tuple(scale.shape) == (Cn,) and tuple(shift.shape) == (Cn,)
    out = torch.empty_like(x)
    _op('dmad_wrn_preact', _ptr(x), _ptr(scale), _ptr(shift), x.numel() // Cn, Cn, _ptr(out))
    return out


def wrn_preact_bwd(g: torch.Tensor, o: torch.Tensor, scale: torch.Tensor, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dmad_wrn_preact_bwd: g, o (the saved post-ReLU map), res (optional) [..., C], scale [C] -> res + (o > 0) * scale * g (test hook)."""
    g, o, scale = _f32(g), _f32(o), _f32(scale)
    Cn = g.shape[-1]
    assert g.is_cuda and o.shape == g.shape and tuple(scale.shape) == (Cn,)
    if res is not None:
        res = _f32(res)
        assert res.shape == g.shape
    gx = torch.empty_like(g)
    _op('dmad_wrn_preact_bwd', _ptr(g), _ptr(o), _ptr(scale), _ptr(res), g.numel() // Cn, Cn, _ptr(gx))
    return gx


def wrn_stem(spec: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """dmad_wrn_stem: spec [B,32,32], w [16,9] -> [B,32,32,16] (the 1 -> 16 3x3 conv, no BN, no ReLU) (test hook)."""
    spec, w = _f32(spec), _f32(w)
    B = spec.shape[0]
    assert spec.is_cuda and tuple(spec.shape) == (B, 32, 32) and tuple(w.shape) == (16, 9)
    out = torch.empty((B, 32, 32, 16), device=spec.device, dtype=torch.float32)
    _op('dmad_wrn_stem', _ptr(spec), _ptr(w), B, _ptr(out))
    return out


def wrn_stem_bwd(g: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """dmad_wrn_stem_bwd: g [B,32,32,16], w [16,9] -> gspec [B,32,32] (the stem conv's backward) (test hook)."""
    g, w = _f32(g), _f32(w)
    B = g.shape[0]
    assert g.is_cuda and tuple(g.shape) == (B, 32, 32, 16) and tuple(w.shape) == (16, 9)
    gspec = torch.empty((B, 32, 32), device=g.device, dtype=torch.float32)
    _op('dmad_wrn_stem_bwd', _ptr(g), _ptr(w), B, _ptr(gspec))
    return gspec


def _dn_pw_image(w: torch.Tensor) -> torch.Tensor:
    """[M, K] -> the 1x1 kernels' image [M, K4]: K rounded up to 4 with zero columns"""
    M, K = w.shape
    A = torch.zeros((M, (K + 3) & ~3), device=w.device, dtype=torch.float32)
    A[:, :K] = w
    return A


def dn_pw(x: torch.Tensor, w: torch.Tensor, s_in: torch.Tensor, b_in: torch.Tensor, s_out: Optional[torch.Tensor] = None,
          b_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dmad_dn_pw: x [n_px, ldx] (a stream: only channels [0, K) are read), w [M, K], s_in / b_in [K], s_out / b_out [M] or None ->
    [n_px, M]: epi(w @ pre(s_in, x, b_in)) (DenseNet's bottleneck / transition 1x1) (test hook)."""
    x, w, s_in, b_in = _f32(x), _f32(w), _f32(s_in), _f32(b_in)
    M, K = w.shape
    assert x.is_cuda and x.dim() == 2 and x.shape[1] >= K and tuple(s_in.shape) == (K,) and tuple(b_in.shape) == (K,)
    if s_out is not None:
        s_out, b_out = _f32(s_out), _f32(b_out)
    out = torch.empty((x.shape[0], M), device=x.device, dtype=torch.float32)
    A = _dn_pw_image(w)
    _op('dmad_dn_pw', _ptr(A), M, K, _ptr(x), x.shape[1], x.shape[0], _ptr(s_in), _ptr(b_in), _ptr(s_out), _ptr(b_out), _ptr(out), M)
    return out


def dn_pw_bwd(g: torch.Tensor, w: torch.Tensor, x: torch.Tensor, s1: torch.Tensor, b1: torch.Tensor, out: torch.Tensor, add: bool = True,
              pool_H: int = 0) -> torch.Tensor:
    """dmad_dn_pw_bwd, IN PLACE on `out`: g [n_px or n_px / 4, ldg] (channels [0, K) are read), w [K, M] in the FORWARD layout (the conv's
    [cout = K, cin = M]), x / out [n_px, ld] streams, s1 / b1 [M] -> out[:, :M] (+)= (pre(s1, x, b1) > 0) * s1 * (g' @ w); pool_H: the
    resolution of out's maps when g is the gradient of their 2x2 average pool (test hook)."""
    g, w, x, s1, b1 = _f32(g), _f32(w), _f32(x), _f32(s1), _f32(b1)
    K, M = w.shape
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 2 and x.dim() == 2 and g.dim() == 2
    assert g.shape[1] >= K and x.shape[1] >= M and out.shape[1] >= M and x.shape[0] == out.shape[0] and tuple(s1.shape) == (M,)
    assert g.shape[0] * (4 if pool_H else 1) == out.shape[0]
    A = _dn_pw_image(w.t().contiguous())
    _op('dmad_dn_pw_bwd', _ptr(A), M, K, _ptr(g), g.shape[1], out.shape[0], 1 if pool_H else 0, int(pool_H) or 2,
        _ptr(x), x.shape[1], _ptr(s1), _ptr(b1), _ptr(out), out.shape[1], 1 if add else 0)
    return out


def dn_growth(h: torch.Tensor, w: torch.Tensor, stream: torch.Tensor, off: int) -> torch.Tensor:
    """dmad_dn_growth, IN PLACE on `stream`: h [B,H,H,48], w [12,48,3,3] -> stream[..., off:off + 12] = conv3x3(h) (zero padding); every
    other channel of stream [B,H,H,ld] is left alone (test hook)."""
    h, w = _f32(h), _f32(w)
    B, H = h.shape[0], h.shape[1]
    assert stream.is_cuda and stream.dtype == torch.float32 and stream.is_contiguous() and tuple(stream.shape[:3]) == (B, H, H)
    assert tuple(h.shape) == (B, H, H, 48) and tuple(w.shape) == (12, 48, 3, 3)
    A = torch.zeros((16, 9, 48), device=h.device, dtype=torch.float32)
    A[:12] = w.reshape(12, 48, 9).permute(0, 2, 1)
    _op('dmad_dn_growth', _ptr(A), _ptr(h), B, H, _ptr(stream), stream.shape[3], int(off))
    return stream


def dn_growth_bwd(g: torch.Tensor, off: int, w: torch.Tensor, h: torch.Tensor, s2: torch.Tensor) -> torch.Tensor:
    """dmad_dn_growth_bwd: g [B,H,H,ld] (the gradient stream; its slice [off, off + 12) is read), w [12,48,3,3], h [B,H,H,48], s2 [48] ->
    gh [B,H,H,48] = (h > 0) * s2 * conv3x3^T(g slice) (test hook)."""
    g, w, h, s2 = _f32(g), _f32(w), _f32(h), _f32(s2)
    B, H = h.shape[0], h.shape[1]
    assert g.is_cuda and tuple(g.shape[:3]) == (B, H, H) and tuple(h.shape) == (B, H, H, 48) and tuple(w.shape) == (12, 48, 3, 3)
    A = w.reshape(12, 48, 9).flip(2).permute(1, 2, 0).contiguous()          # [c][8 - tap][j]
    gh = torch.empty_like(h)
    _op('dmad_dn_growth_bwd', _ptr(A), _ptr(g), g.shape[3], int(off), _ptr(h), _ptr(s2), B, H, _ptr(gh))
    return gh


def dn_stem(spec: torch.Tensor, w: torch.Tensor, stream: torch.Tensor) -> torch.Tensor:
    """dmad_dn_stem, IN PLACE on `stream`: spec [B,32,32], w [24,9] -> stream[..., :24] of [B,32,32,ld] (test hook)."""
    spec, w = _f32(spec), _f32(w)
    B = spec.shape[0]
    assert stream.is_cuda and stream.dtype == torch.float32 and stream.is_contiguous() and tuple(stream.shape[:3]) == (B, 32, 32) and tuple(w.shape) == (24, 9)
    _op('dmad_dn_stem', _ptr(spec), _ptr(w), B, _ptr(stream), stream.shape[3])
    return stream


def dn_stem_bwd(g: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """dmad_dn_stem_bwd: g [B,32,32,ld] (channels [0, 24) are read), w [24,9] -> gspec [B,32,32] (test hook)."""
    g, w = _f32(g), _f32(w)
    B = g.shape[0]
    assert g.is_cuda and tuple(g.shape[:3]) == (B, 32, 32) and tuple(w.shape) == (24, 9)
    gspec = torch.empty((B, 32, 32), device=g.device, dtype=torch.float32)
    _op('dmad_dn_stem_bwd', _ptr(g), g.shape[3], _ptr(w), B, _ptr(gspec))
    return gspec


def dn_pool(t: torch.Tensor, C: int, out: torch.Tensor) -> torch.Tensor:
    """dmad_dn_pool, IN PLACE on `out`: t [B,H,H,ldt] -> out[..., :C] of [B,H/2,H/2,ldo], the 2x2 average pool of t's first C channels (test hook)."""
    t = _f32(t)
    B, H = t.shape[0], t.shape[1]
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape[:3]) == (B, H // 2, H // 2)
    _op('dmad_dn_pool', _ptr(t), t.shape[3], B, H, int(C), _ptr(out), out.shape[3])
    return out


def dn_preact(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """dmad_dn_preact: x [n_px, ldx], scale / shift [C] -> [n_px, C]: DenseNet's one pre-activation function on x's first C channels (test hook)."""
    x, scale, shift = _f32(x), _f32(scale), _f32(shift)
    Cn = scale.shape[0]
    assert x.is_cuda and x.dim() == 2 and x.shape[1] >= Cn
    out = torch.empty((x.shape[0], Cn), device=x.device, dtype=torch.float32)
    _op('dmad_dn_preact', _ptr(x), x.shape[1], _ptr(scale), _ptr(shift), x.shape[0], Cn, _ptr(out))
    return out


def dn_head(x: torch.Tensor, bns: torch.Tensor, bnb: torch.Tensor, fcw: torch.Tensor, fcb: torch.Tensor) -> torch.Tensor:
    """dmad_dn_head: x [B,HW,ldx], bns / bnb [C], fcw [ncls,C], fcb [ncls] -> logits [B,ncls] (test hook)."""
    x, bns, bnb, fcw, fcb = _f32(x), _f32(bns), _f32(bnb), _f32(fcw), _f32(fcb)
    B, HW, ldx = x.shape
    ncls, Cn = fcw.shape
    out = torch.empty((B, ncls), device=x.device, dtype=torch.float32)
    _op('dmad_dn_head', _ptr(x), ldx, _ptr(bns), _ptr(bnb), _ptr(fcw), _ptr(fcb), B, HW, Cn, ncls, _ptr(out))
    return out


def dn_head_bwd(g_logits: torch.Tensor, fcws: torch.Tensor, x: torch.Tensor, bns: torch.Tensor, bnb: torch.Tensor, ldg: int) -> torch.Tensor:
    """dmad_dn_head_bwd: g_logits [B,ncls], fcws [ncls,C], x [B,HW,ldx] -> g [B,HW,ldg] with channels [0, C) written, the rest zero (test hook)."""
    g_logits, fcws, x, bns, bnb = _f32(g_logits), _f32(fcws), _f32(x), _f32(bns), _f32(bnb)
    B, HW, ldx = x.shape
    ncls, Cn = fcws.shape
    g = torch.zeros((B, HW, int(ldg)), device=x.device, dtype=torch.float32)
    _op('dmad_dn_head_bwd', _ptr(g_logits), _ptr(fcws), _ptr(x), ldx, _ptr(bns), _ptr(bnb), B, HW, Cn, ncls, _ptr(g), int(ldg))
    return g


def rx_conv1_bwd(g: torch.Tensor, a: torch.Tensor, w: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """dmad_rx_conv1_bwd: g, a [B,32,32,64], w [64,9], scale [64] -> gspec [B,32,32] (conv1's ReLU, BN and 1 <- 64 conv backward) (test hook)."""
    g, a, w, scale = _f32(g), _f32(a), _f32(w), _f32(scale)
    B = g.shape[0]
    assert tuple(g.shape) == (B, 32, 32, 64) and tuple(a.shape) == (B, 32, 32, 64) and tuple(w.shape) == (64, 9) and tuple(scale.shape) == (64,)
    gspec = torch.empty((B, 32, 32), device=g.device, dtype=torch.float32)
    _op('dmad_rx_conv1_bwd', _ptr(g), _ptr(a), _ptr(w), _ptr(scale), B, _ptr(gspec))
    return gspec


# ---------------------------------------------------------------------- which engine a module binds to
def bind_classifier(state_dict, loader_name: str, engine: Optional[Engine] = None) -> Engine:
    """Engine that holds exactly `state_dict` as its classifier: `engine` (refused if it holds another one), else the
    shared engine, else — when the shared engine already serves a different classifier — an engine of this module's own
    (classifier-only use: mel + classify; the fused Monte Carlo loop needs denoiser and classifier in ONE engine)."""
    if engine is not None:
        engine.bind('classifier', state_dict, getattr(engine, loader_name))
        return engine
    eng = get_engine()
    if eng.has_classifier and eng.classifier_owner != state_fingerprint(state_dict):
        eng = Engine(dict(eng.wavenet_geometry), max_batch=eng.max_batch, precision=eng.precision)
    eng.bind('classifier', state_dict, getattr(eng, loader_name))
    return eng


def bind_m5(state_dict, stride: int = 16, engine: Optional[Engine] = None) -> Engine:
    """Engine that holds exactly `state_dict` as its M5 part: `engine` (refused if it holds another M5), else the shared engine (so
    that a DiffWave purifier and M5 meet in ONE engine and a query is one call), else -- when the shared engine already serves a
    different M5 -- an engine of this module's own."""
    eng = engine if engine is not None else get_engine()
    if engine is None and eng.has_m5 and eng.m5_owner != state_fingerprint(state_dict):
        eng = Engine(dict(eng.wavenet_geometry), max_batch=eng.max_batch, precision=eng.precision)
    eng.bind('m5', state_dict, lambda sd: eng.load_m5(sd, stride))
    return eng


def bind_kws(state_dict, kernel_size=(20, 5), stride=(8, 2), engine: Optional[Engine] = None) -> Engine:
    """Engine that holds exactly `state_dict` as its KWS part, chosen as bind_m5 chooses: `engine` (refused if it holds another KWS
    model), else the shared engine, else -- when the shared engine already serves a different one -- an engine of this module's own."""
    eng = engine if engine is not None else get_engine()
    if engine is None and eng.has_kws and eng.kws_owner != state_fingerprint(state_dict):
        eng = Engine(dict(eng.wavenet_geometry), max_batch=eng.max_batch, precision=eng.precision)
    eng.bind('kws', state_dict, lambda sd: eng.load_kws(sd, kernel_size, stride))
    return eng


_ENGINES: Dict[tuple, Engine] = {}
_PRECISIONS = {'bf16': BF16, 'fp32': FP32, 'exact': EXACT}


def get_engine(wavenet_config: Optional[dict] = None, precision: Optional[int] = None, max_batch: Optional[int] = None,
               fresh: bool = False) -> Engine:
    """Process-wide engine per (device, precision), shared by the denoiser, the mel transform and the classifier so that
    the Monte Carlo loop can run fused.  Defaults: DMAD_PRECISION = exact (bf16 throughput + fp32 recheck of the close
    votes: counts equal the fp32 path's; bf16 and fp32 are opt-in), DMAD_MAX_BATCH = 64.  A caller that names a WaveNet
    geometry or a max_batch the shared engine was not created with gets a DmadError, never another model's engine.
    Engines are single-stream objects (the step-embedding cache is not stream-keyed): one HIP stream at a time."""
    if precision is None:
        precision = _PRECISIONS[os.environ.get('DMAD_PRECISION', 'exact').lower()]
    key = (torch.cuda.current_device() if torch.cuda.is_available() else -1, precision)
    if fresh or key not in _ENGINES:
        eng = Engine(wavenet_config, max_batch=max_batch if max_batch is not None else int(os.environ.get('DMAD_MAX_BATCH', '64')),
                     precision=precision)
        if fresh:
            return eng
        _ENGINES[key] = eng
        return eng
    eng = _ENGINES[key]
    if wavenet_config is not None:
        want = Engine.geometry(wavenet_config)
        if want != eng.wavenet_geometry:
            raise DmadError('the shared engine was created for WaveNet geometry %s, not %s: create the denoiser first or pass '
                            'an engine of its own (get_engine(..., fresh=True))' % (eng.wavenet_geometry, want))
    if max_batch is not None and max_batch != eng.max_batch:
        raise DmadError('the shared engine has max_batch %d, not %d (set DMAD_MAX_BATCH or use fresh=True)' % (eng.max_batch, max_batch))
    return eng
