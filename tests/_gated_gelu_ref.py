"""fp64 reference and DERIVED element-wise bound of GEMM mode 5, gelu(gate) * up (csrc/enc_gemm.hip, CRS_ENC_GATED_GELU), on the
terms of tests/_gated_ref.py with the SiLU error replaced by the erf GELU's.  Needs no device.

    out[m, j] = fp16( gelu(acc[m, g] + b[g]) * (acc[m, g + 16] + b[g + 16]) ),   g = 32 (j // 16) + j % 16,   gelu(x) = x Phi(x)

  e_G, e_V   as _gated_ref: 2 K u S + 2 u (S + |b|) per column
  gelu       |gelu'(x)| = |Phi(x) + x phi(x)| <= 1.13 (its maximum is 1.1290 at x = sqrt 2), so the input error moves the value by at
             most 1.13 e_G.  The kernel's evaluation (csrc/enc_gelu.h: a rational fit of erf on z clamped to [-4, 4]) states
             |gelu error| <= 1.4e-6 over [-6, 6]; beyond, erf is +-1 to fp32 and the value is 0.5 x (1 + erf): three roundings, taken
             as 8 u |x| everywhere on top of the stated figure:      e_s = 1.13 e_G + 1.4e-6 + 8 u (|G| + e_G)
  product    as _gated_ref: |s| e_V + (|V| + e_V) e_s, one fp32 rounding (2 u relative), half an fp16 ulp.
"""
import math

import torch

import _gated_ref as gt
import _gemm_ref as gr

U, BLOCK = gr.U, gt.BLOCK
GELU_SLOPE = 1.13
GELU_ABS = 1.4e-6         # csrc/enc_gelu.h's stated |gelu error|
FAULTS = ("silu_for_gelu", "swapped")


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def ref_and_bound(a, w, bias, ps=None):
    """(ref, bound) fp64 [m, F] of mode 5 for interleaved w [2F, K] and bias [2F] (or None)."""
    k = a.shape[1]
    f = w.shape[0] // 2
    p, s = ps or gr.products(a, w, 1)
    p, s = p[0], s[0]
    e = 2.0 * k * U * s
    if bias is not None:
        b = bias.double()[None, :]
        p = p + b
        e = e + 2.0 * U * (s + b.abs())
    j = torch.arange(f)
    g = 2 * BLOCK * (j // BLOCK) + j % BLOCK
    G, V, eG, eV = p[:, g], p[:, g + BLOCK], e[:, g], e[:, g + BLOCK]
    sg = gelu64(G)
    ref = sg * V
    e_s = GELU_SLOPE * eG + GELU_ABS + 8.0 * U * (G.abs() + eG)
    err = sg.abs() * eV + (V.abs() + eV) * e_s
    err = err + 2.0 * U * (ref.abs() + err)
    return ref, err + gr.half_ulp16(ref.abs() + err)


def emulate(a, w, bias, fault=None, step=16):
    """A mode-5 kernel in fp32 on the CPU (_gated_ref.emulate's accumulation, torch's fp32 erf GELU).  fault: SiLU in place of GELU
    (mode 4's epilogue); the two halves read in the other order.  (The tanh approximation of GELU differs from the erf form by
    less than the fp16 rounding of these outputs: no element-wise bound on fp16 outputs can tell them apart, and none is claimed.)"""
    acc = gr.emulate(a, w, None, None, 3, slabs=1, step=step)[0]
    if bias is not None:
        acc = acc + bias.float()[None, :]
    f = w.shape[0] // 2
    j = torch.arange(f)
    g = 2 * BLOCK * (j // BLOCK) + j % BLOCK
    v = g + BLOCK
    if fault == "swapped":
        g, v = v, g
    G, V = acc[:, g], acc[:, v]
    if fault == "silu_for_gelu":
        act = G * torch.sigmoid(G)
    else:
        act = torch.nn.functional.gelu(G)
    return (act * V).half()
