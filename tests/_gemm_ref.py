"""fp64 references and DERIVED error bounds for the encoder's GEMM kernels on their own (csrc/enc_gemm*.hip, enc_rowln.hip), shared by
tests/test_gemm_ref_cpu.py, test_gemm_families_gpu.py and test_proj_ln_gpu.py.  Needs no device: torch on the CPU only.

    C = epilogue(A[M, K] W[N, K]^T)      A, W fp16; mode 0: + bias -> fp16; 1: + bias, erf-GELU -> fp16; 2: + bias + residual -> fp32;
                                         3: raw fp32 partial products, out[slabs][M][N]

The reference is the fp64 product of the fp16 operand VALUES.  For element (i, j) let S = sum_k |a_ik| |w_jk| over the columns its
accumulator saw, K_s their count, u = 2^-24.  None of the bounds below is fitted to what a kernel gives:

  accumulator   E = 2 K_s u S.  fp16 x fp16 products are exact in fp32 (22 significant bits); each of the K_s additions errs by at
                most one fp32 ulp (2u relative) of a partial sum that is at most S in magnitude -- whatever rounding the MFMA uses
                inside, in any order, so one formula covers every tile shape and every split of K.
  bias          + 2u (S + |bias|)            (modes 0 / 1 / 2, when there is a bias: one more fp32 addition)
  residual      + 2u (S + |bias| + |res|)    (mode 2)
  mode 0        + half an fp16 ulp of (|ref| + E): the output rounding, subnormal-aware (fp16: ulp 2^(e - 10), 2^-24 below 2^-14)
  mode 1        1.13 E_pre + 1.4e-6 + half an fp16 ulp: 1.13 bounds |gelu'|, 1.4e-6 is csrc/enc_gelu.h's stated error of its erf
                (tests/test_encoder_hard_gpu.py::test_gelu_epilogue_against_fp64_erf holds it to that)
  mode 3        every slab against ITS partial product.  Both split-K layouts give slab z the columns [z K / slabs, (z + 1) K / slabs):
                  panel (gemm_panel_kernel<3, TM>): workgroup z = blockIdx.z walks kin chunks of kc columns from (z kin) kc on, and
                    kin kc slabs = K (GemmPlan) -- the describe line's grid is NBxMBxslabs;
                  gemm8 (gemm8_kernel<3, false, V>): item (tile, z) contracts [z ksplit, (z + 1) ksplit), ksplit = K / slabs -- the
                    describe line's grid is (tiles x slabs)x1x1.
                slab_ranges() states it; the GPU tests assert the grid's slab factor from the describe text.
  proj_ln       y = A W^T + bias + x32 (pre-LayerNorm), out = g (y - mean) / sigma + b, sigma = sqrt(var + eps).  With s slabs of K / s
                columns the pre-LN error is E = 2 (K / s) u S + 2 (s - 1) u S (summing the slabs) + the bias and residual terms above
                (s = 1: the fused kernel and the mode-2 GEMM).  To first order an error e_ij of y moves out_ij by
                g_j / sigma_i (e_ij - mean_j e_ij - xhat_ij mean_j (xhat_ij e_ij)), so
                  |d out_ij| <= |g_j| / sigma_i (E_ij + mean_j E_ij + |xhat_ij| sqrt(mean_j E_ij^2))        (Cauchy-Schwarz, mean xhat^2 <= 1)
                plus a = 4 max |torch fp32 LayerNorm - fp64 LayerNorm| on the same pre-LN input (the accumulation-order rule of
                tests/_encoder_cases.py: the kernel's fp32 statistics may sum in another order than torch's), plus half an fp16 ulp for
                x16.  The second-order term, (1 + |xhat|) |g| (max_j E_ij / sigma_i)^2, must stay below 1 % of the bound: proj_ln_bound
                returns it and the tests assert it (a case that fails it is inadmissible and gets re-drawn, not a wider bound).
"""
import math

import torch

U = 2.0 ** -24
GELU_ERR = 1.4e-6        # csrc/enc_gelu.h
GELU_SLOPE = 1.13        # max |gelu'|


def half_ulp16(x):
    """half an fp16 ulp at magnitude |x| (fp64 tensor): normal 2^(e - 10), subnormal range 2^-24"""
    expo = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -14)))
    return 0.5 * torch.pow(2.0, expo - 10)


def distinct(v):
    """v (1-d fp32) with equal values nudged apart by an ulp: a wrong column cannot hide behind an equal value (among 8320 normal
    draws a pair of equal fp32 values is likely)"""
    v = v.clone()
    for _ in range(64):
        s, idx = torch.sort(v)
        eq = torch.nonzero(s[1:] == s[:-1]).flatten()
        if eq.numel() == 0:
            return v
        v[idx[eq + 1]] = torch.nextafter(s[eq + 1], torch.tensor(float("inf")))
    raise AssertionError("values still not distinct")


def make_inputs(m, n, k, seed=None):
    """a ~ 0.5 N(0, 1) fp16 [m, k], w ~ 0.05 N(0, 1) fp16 [n, k], bias 0.1 N(0, 1) fp32 [n], residual N(0, 1) fp32 [m, n] (CPU), as
    tests/test_encoder_gpu.py::test_gemm_vs_torch_fp32 draws them; bias values and residual columns pairwise distinct."""
    g = torch.Generator().manual_seed(m * 7 + n if seed is None else seed)
    a = (torch.randn((m, k), generator=g) * 0.5).half()
    w = (torch.randn((n, k), generator=g) * 0.05).half()
    bias = distinct(torch.randn(n, generator=g) * 0.1)
    res = torch.randn((m, n), generator=g)
    res[0] = distinct(res[0])                 # columns that differ in their first row are pairwise distinct
    assert torch.unique(bias).numel() == n and torch.unique(res[0]).numel() == n
    return a, w, bias, res


def slab_ranges(k, slabs):
    """columns of K that slab z of a mode-3 launch contracts (both the panel's and gemm8's layout, see the module text)"""
    assert k % slabs == 0
    ks = k // slabs
    return [(z * ks, (z + 1) * ks) for z in range(slabs)]


def products(a, w, slabs=1):
    """fp64 P[slabs, m, n] and S[slabs, m, n] = sum |a| |w| per slab"""
    a64, w64 = a.double(), w.double()
    ps, ss = [], []
    for lo, hi in slab_ranges(a.shape[1], slabs):
        ps.append(a64[:, lo:hi] @ w64[:, lo:hi].T)
        ss.append(a64[:, lo:hi].abs() @ w64[:, lo:hi].abs().T)
    return torch.stack(ps), torch.stack(ss)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gemm_ref_and_bound(a, w, bias, res, mode, slabs=1, ps=None):
    """(ref, bound), fp64: [m, n] for modes 0 / 1 / 2 (whole K: slabs is ignored), [slabs, m, n] for mode 3.  bias may be None.
    ps: products(a, w, slabs of a mode-3 case, else 1) where the caller shares them among cases."""
    k = a.shape[1]
    if mode == 3:
        p, s = ps or products(a, w, slabs)
        return p, 2.0 * (k // slabs) * U * s
    p, s = ps or products(a, w, 1)
    p, s = p[0], s[0]
    e = 2.0 * k * U * s
    pre = p
    if bias is not None:
        b = bias.double()[None, :]
        pre = pre + b
        e = e + 2.0 * U * (s + b.abs())
    babs = bias.double().abs()[None, :] if bias is not None else 0.0
    if mode == 2:
        r = res.double()
        return pre + r, e + 2.0 * U * (s + babs + r.abs())
    if mode == 0:
        return pre, e + half_ulp16(pre.abs() + e)
    assert mode == 1
    ref = gelu64(pre)
    err = GELU_SLOPE * e + GELU_ERR
    return ref, err + half_ulp16(ref.abs() + err)


def layer_norm64(y, g, b, eps):
    mean = y.mean(1, keepdim=True)
    var = ((y - mean) ** 2).mean(1, keepdim=True)
    sigma = torch.sqrt(var + eps)
    xhat = (y - mean) / sigma
    return xhat * g.double()[None, :] + b.double()[None, :], xhat, sigma


def proj_ln_ref_and_bound(a, w, bias, res, g, b, eps, slabs=1, ps=None):
    """fp64 reference of LayerNorm(a w^T + bias + res) and the bounds of x32 and x16 (module text).  Returns
    (ref, bound32, bound16, second_order_ratio, a_term)."""
    k = a.shape[1]
    p, s = ps or products(a, w, 1)
    p, s = p[0], s[0]
    babs, r = bias.double().abs()[None, :], res.double()
    y = p + bias.double()[None, :] + r
    e = 2.0 * (k // slabs) * U * s + 2.0 * (slabs - 1) * U * s + 2.0 * U * (s + babs) + 2.0 * U * (s + babs + r.abs())
    ref, xhat, sigma = layer_norm64(y, g, b, eps)
    gabs = g.double().abs()[None, :]
    first = gabs / sigma * (e + e.mean(1, keepdim=True) + xhat.abs() * torch.sqrt((e ** 2).mean(1, keepdim=True)))
    # the accumulation-order term: torch's fp32 LayerNorm against fp64 on the SAME fp32 pre-LN input
    y32 = y.float()
    ln32 = torch.nn.functional.layer_norm(y32, (y32.shape[1],), g.float(), b.float(), eps).double()
    a_term = 4.0 * (ln32 - layer_norm64(y32.double(), g, b, eps)[0]).abs().max().item()
    bound32 = first + a_term
    second = (1.0 + xhat.abs()) * gabs * (e.max(1, keepdim=True).values / sigma) ** 2
    bound16 = bound32 + half_ulp16(ref.abs() + bound32)
    return ref, bound32, bound16, (second / bound32).max().item(), a_term


def ratio(out, ref, bound):
    """largest |out - ref| / bound over the elements (fp64); the tests assert <= 1"""
    return ((out.double() - ref).abs() / bound).max().item()


# ---- an fp32 emulation of the kernels' order, with the faults the bound must catch (tests/test_gemm_ref_cpu.py) ------------------------
def gelu_tanh32(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


FAULTS = {                      # name -> modes it applies to
    "drop_last_k16": (0, 1, 2, 3),      # (a) the last 16 columns of K dropped for the rows of the last ragged row tile
    "bias_next_col": (0, 1, 2),         # (b) the bias of column j + 1 used for the last 32 columns
    "clamped_rows": (0, 1, 2, 3),       # (c) rows past the last whole row tile take row M - 1's result
    "slab_neighbour": (3,),             # (d) one slab computed over the neighbouring K chunk
    "tanh_gelu": (1,),                  # (e) tanh-GELU in place of erf-GELU
    "residual_stride": (2,),            # (f) a residual row read with stride N + 4
}


def emulate(a, w, bias, res, mode, slabs=1, fault=None, tile_m=128, step=16):
    """What a kernel computes, in fp32 on the CPU: the contraction accumulated `step` columns at a time (one MFMA's depth) in fp32,
    then the epilogue in fp32 and the output rounding.  fault: a key of FAULTS, planted as a kernel would commit it."""
    m, k = a.shape
    n = w.shape[0]
    a32, w32 = a.float(), w.float()
    last_tile = (m - 1) // tile_m * tile_m                 # first row of the last (ragged) row tile
    whole = m // tile_m * tile_m                           # rows of whole tiles

    def contract(lo, hi, rows_short=None):
        acc = torch.zeros((m, n), dtype=torch.float32)
        for k0 in range(lo, hi, step):
            part = a32[:, k0:k0 + step] @ w32[:, k0:k0 + step].T
            if rows_short is not None and k0 + step > hi - 16:
                part[rows_short:] = 0.0
            acc = acc + part
        return acc

    out = []
    for z, (lo, hi) in enumerate(slab_ranges(k, slabs if mode == 3 else 1)):
        if fault == "slab_neighbour" and z == 0:
            lo, hi = hi, 2 * hi - lo                       # slab 0 reads slab 1's columns
        short = last_tile if (fault == "drop_last_k16" and hi == k) else None
        acc = contract(lo, hi, short)
        if fault == "clamped_rows" and whole < m:
            acc[whole:] = acc[m - 1]
        out.append(acc)
    if mode == 3:
        return torch.stack(out)
    acc = out[0]
    if bias is not None:
        bcol = bias.float().clone()
        if fault == "bias_next_col":
            bcol[-32:] = torch.roll(bias.float(), -1)[-32:]
        acc = acc + bcol[None, :]
    if mode == 2:
        r = res.float()
        if fault == "residual_stride":                      # row i read at i (N + 4) instead of i N, from row 1 on
            flat = torch.cat([r.flatten(), r.flatten()[:4 * m + n]])
            r = torch.stack([flat[i * (n + 4):i * (n + 4) + n] for i in range(m)])
        return acc + r
    if mode == 1:
        acc = gelu_tanh32(acc) if fault == "tanh_gelu" else torch.nn.functional.gelu(acc)
    return acc.half()
