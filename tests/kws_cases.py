"""Shared by tests/test_kws_cpu.py and tests/test_gpu_kws.py: the fixture tests/golden/kws_vanilla.npz (make_golden_kws.py) and kws_walk, a
float64 walk through the attention-CRNN keyword spotter with the GRU cell written out step by step and a hand-written backward.  It
shares no code with nn.GRU or autograd, returns every stage dmad_kws_tape can read back, and is the GPU tests' reference once the CPU
test has proved it against the fixture."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kws_vanilla.npz')
CASES = (5, 20, 21, 37, 81, 501)
HID = 64


@functools.lru_cache(maxsize=1)
def fixture():
    """the whole fixture as a dict of read-only numpy arrays"""
    with np.load(GOLDEN) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def state_dict(dtype=torch.float32):
    """the 24 tensors in the state dict's order"""
    fx = fixture()
    return {str(k): torch.from_numpy(fx['w.' + str(k)].copy()).to(dtype) for k in fx['keys']}


def steps(T):
    return ((T - 5) // 2) // 8 + 1


def support(T):
    """bool [T]: the frames 16 j .. 16 j + 4, j < steps(T), that some GRU step reads"""
    m = np.zeros(T, dtype=bool)
    for j in range(steps(T)):
        m[16 * j:16 * j + 5] = True
    return m


def _sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


def _gru_dir(inp, wih, whh, bih, bhh, reverse):
    """one direction of one layer: inp [B,S,K] -> (h [B,S,64], the per-step tape)"""
    B, S, _ = inp.shape
    h = inp.new_zeros(B, HID)
    out, tape = [None] * S, [None] * S
    for t in (range(S - 1, -1, -1) if reverse else range(S)):
        gi = inp[:, t] @ wih.T + bih
        gh = h @ whh.T + bhh
        r = _sig(gi[:, :HID] + gh[:, :HID])
        z = _sig(gi[:, HID:2 * HID] + gh[:, HID:2 * HID])
        n = torch.tanh(gi[:, 2 * HID:] + r * gh[:, 2 * HID:])
        tape[t] = (h, r, z, n, gh[:, 2 * HID:])
        h = (1 - z) * n + z * h
        out[t] = h
    return torch.stack(out, dim=1), tape


def _gru_dir_back(g_out, tape, inp, wih, whh, reverse):
    """g_out [B,S,64] at the direction's output -> the gradient at inp [B,S,K]"""
    B, S, _ = g_out.shape
    g_inp = torch.zeros_like(inp)
    carry = g_out.new_zeros(B, HID)
    for t in (range(S) if reverse else range(S - 1, -1, -1)):          # the forward's order, backwards
        h_prev, r, z, n, ghn = tape[t]
        dh = g_out[:, t] + carry
        dn_pre = dh * (1 - z) * (1 - n * n)
        dz_pre = dh * (h_prev - n) * z * (1 - z)
        dr_pre = dn_pre * ghn * r * (1 - r)
        g_inp[:, t] = torch.cat([dr_pre, dz_pre, dn_pre], dim=1) @ wih
        carry = dh * z + torch.cat([dr_pre, dz_pre, dn_pre * r], dim=1) @ whh
    return g_inp


def kws_walk(sd, spec, g_logp=None, dtype=torch.float64):
    """sd: the state dict; spec [B,32,T] or [B,1,32,T]; -> dict of `dtype` (float64) tensors: 'x0' [B,S,64] (sepconv output), 'h0' / 'h1' [B,S,128]
    (GRU layer outputs, forward direction first), 'e' [B,S] (attention scores), 'logp' [B,4] and, with g_logp [B,4], 'g_spec' [B,32,T].  dtype = torch.float32 gives the same walk's own
    float32 error, the scale the engine's stages are measured with"""
    w = {k: v.detach().to(dtype).cpu() for k, v in sd.items()}
    x = spec.detach().to(dtype).cpu()
    x = x[:, 0] if x.dim() == 4 else x
    B, C, T = x.shape
    S = steps(T)
    P = 'CRNN_model.'
    dw, dwb = w[P + 'sepconv.0.weight'][:, 0], w[P + 'sepconv.0.bias']             # [32,5]
    pw, pwb = w[P + 'sepconv.1.weight'][:, :, 0], w[P + 'sepconv.1.bias']          # [64,32]
    frames = torch.stack([x[:, :, 16 * j:16 * j + 5] for j in range(S)], dim=1)    # [B,S,32,5]: all that is ever read
    d = (frames * dw).sum(-1) + dwb                                                # [B,S,32]
    x0 = d @ pw.T + pwb
    layers, inp = [], x0
    for l in range(2):
        dirs = []
        for sfx in ('', '_reverse'):
            p = [w['%sgru.%s_l%d%s' % (P, k, l, sfx)] for k in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
            h, tape = _gru_dir(inp, *p, reverse=bool(sfx))
            dirs.append((h, tape, p))
        layers.append((inp, dirs))
        inp = torch.cat([dirs[0][0], dirs[1][0]], dim=2)
    h0 = layers[1][0]
    h1 = inp
    wx, wxb, vt, u = w['attn_layer.Wx_b.weight'], w['attn_layer.Wx_b.bias'], w['attn_layer.Vt.weight'][0], w['apply_attn.U.weight']
    a_units = torch.tanh(h1 @ wx.T + wxb)                                           # [B,S,128]
    e = a_units @ vt
    ex = torch.exp(e - e.max(dim=1, keepdim=True).values)
    a = ex / ex.sum(dim=1, keepdim=True)
    ctx = (a.unsqueeze(2) * h1).sum(dim=1)                                         # [B,128]
    zl = ctx @ u.T
    m = zl.max(dim=1, keepdim=True).values
    logp = zl - (m + torch.log(torch.exp(zl - m).sum(dim=1, keepdim=True)))
    out = {'x0': x0, 'h0': h0, 'h1': h1, 'e': e, 'logp': logp}
    if g_logp is None:
        return out
    g = g_logp.detach().to(dtype).cpu()
    g_z = g - torch.exp(logp) * g.sum(dim=1, keepdim=True)
    g_ctx = g_z @ u
    g_a = (h1 * g_ctx.unsqueeze(1)).sum(dim=2)                                     # [B,S]
    g_h1 = a.unsqueeze(2) * g_ctx.unsqueeze(1)
    g_e = a * (g_a - (a * g_a).sum(dim=1, keepdim=True))
    g_pre = g_e.unsqueeze(2) * vt * (1 - a_units * a_units)
    g_h = g_h1 + g_pre @ wx
    for l in (1, 0):
        inp_l, dirs = layers[l]
        g_in = torch.zeros_like(inp_l)
        for k, (h, tape, p) in enumerate(dirs):
            g_in = g_in + _gru_dir_back(g_h[..., k * HID:(k + 1) * HID], tape, inp_l, p[0], p[1], reverse=bool(k))
        g_h = g_in
    g_d = g_h @ pw                                                                  # [B,S,32]
    g_spec = torch.zeros_like(x)
    for j in range(S):
        g_spec[:, :, 16 * j:16 * j + 5] = g_d[:, j].unsqueeze(2) * dw
    out['g_spec'] = g_spec
    return out
