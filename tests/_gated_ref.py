"""fp64 reference and DERIVED element-wise bound of the gated GEMM epilogue (mode 4, csrc/enc_gemm.hip), on tests/_gemm_ref.py's
terms.  Needs no device.

    out[m, j] = fp16( silu(acc[m, g] + b[g]) * (acc[m, g + 16] + b[g + 16]) ),   g = 32 (j // 16) + j % 16
    W fp16 [2F, K] with gate / up rows interleaved in blocks of 16 (include/crs_encoder.h: CRS_ENC_GATED_SILU), out fp16 [M, F]

With G, V the fp64 pre-activations of the gate and the up column (products of the fp16 operand VALUES + bias), s = silu(G), the
reference is s V.  u = 2^-24.  Nothing below is fitted to what a kernel gives:

  e_G, e_V   _gemm_ref's accumulator and bias terms of the two columns: 2 K u S + 2 u (S + |b|)
  silu       |silu'| <= 1.1 (its maximum is 1.0998 at x = 2.4), so the input error moves s by at most 1.1 e_G.  The kernel evaluates
             x * rcp(1 + exp2(-x log2 e)) in fp32: the argument's two roundings move exp by 2 u |x| relative, v_exp_f32 and
             v_rcp_f32 err by one ulp (2 u) each, the sum and the product by u each -- 2 u |x| + 6 u relative; the bound takes
             8 u (1 + |x|), and |silu(x)| <= |x|:     e_s = 1.1 e_G + 8 u (1 + |G| + e_G) (|G| + e_G)
  product    |s^ V^ - s V| <= |s| e_V + (|V| + e_V) e_s, one fp32 rounding of the product (2 u relative), then half an fp16 ulp.
"""
import torch

import _gemm_ref as gr

U = gr.U
SILU_SLOPE = 1.1
BLOCK = 16


def gate_col(j):
    """column of W's 2F interleaved rows that holds output column j's gate; its up value sits BLOCK columns on"""
    return 2 * BLOCK * (j // BLOCK) + j % BLOCK


def interleave(gate, up):
    """torch [F, ...] x 2 -> [2F, ...] in the header's layout, by its index formula (not the package's helper)"""
    f = gate.shape[0]
    out = torch.empty((2 * f,) + tuple(gate.shape[1:]), dtype=gate.dtype)
    j = torch.arange(f)
    g = 2 * BLOCK * (j // BLOCK) + j % BLOCK
    out[g], out[g + BLOCK] = gate, up
    return out


def make_inputs(m, f, k, seed=None):
    """a fp16 [m, k], interleaved w fp16 [2f, k] and bias fp32 [2f], drawn as _gemm_ref.make_inputs draws them (n = 2 f)"""
    a, w, bias, _ = gr.make_inputs(m, 2 * f, k, seed)
    return a, w, bias


def silu64(x):
    return x * torch.sigmoid(x)


def gated_ref_and_bound(a, w, bias, ps=None):
    """(ref, bound) fp64 [m, F] of mode 4 for interleaved w [2F, K] and bias [2F] (or None)."""
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
    sg = silu64(G)
    ref = sg * V
    e_s = SILU_SLOPE * eG + 8.0 * U * (1.0 + G.abs() + eG) * (G.abs() + eG)
    err = sg.abs() * eV + (V.abs() + eV) * e_s
    err = err + 2.0 * U * (ref.abs() + err)
    return ref, err + gr.half_ulp16(ref.abs() + err)


FAULTS = ("swapped", "silu_wrong_half", "bias_dropped", "pair_next_block")


def emulate(a, w, bias, fault=None, step=16):
    """What a mode-4 kernel computes, in fp32 on the CPU: _gemm_ref.emulate's accumulation (mode 3, one slab: the raw fp32
    product), the bias, SiLU and the product in fp32, one rounding to fp16.  fault: one of FAULTS, planted as a kernel would
    commit it -- the two 16-column halves of a block read in the other order; SiLU applied to the up half; the bias not added;
    a block's gate paired with the NEXT block's up columns."""
    acc = gr.emulate(a, w, None, None, 3, slabs=1, step=step)[0]
    if bias is not None and fault != "bias_dropped":
        acc = acc + bias.float()[None, :]
    f = w.shape[0] // 2
    j = torch.arange(f)
    g = 2 * BLOCK * (j // BLOCK) + j % BLOCK
    v = g + BLOCK
    if fault == "swapped":
        g, v = v, g
    if fault == "pair_next_block":
        v = (v + 2 * BLOCK) % (2 * f)
    G, V = acc[:, g], acc[:, v]
    if fault == "silu_wrong_half":
        return (G * (V * torch.sigmoid(V))).half()
    return ((G * torch.sigmoid(G)) * V).half()
