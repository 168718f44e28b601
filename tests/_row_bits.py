"""The cases of the recorded row-build pin (tests/golden/row_build_bits.npz), shared by tools/ab_row_build.py, which records them,
and tests/test_row_build_bits_gpu.py, which replays them.

A persisted store mixes rows written by different builds of the library, and "an updated row equals the same vector appended" has
to hold across them: the bits a row writer produces are part of the store's format.  The other build tests compare the kernel with
fp64 or with itself; this pin compares it with what the library wrote when the fixture was recorded.

A case is (kind, slab type, dim, R): 5 rows of the kinds the build tests use (tests/_slab_ref.make_rows: gaussian, zero, wide, tiny,
one-hot; tests/_space_build_ref.make_space_rows: random, top, axis, zero, wide) appended at row 0 of zeroed arrays of 5 rows, the
row error starting from 0.
  cos   crs_slab_append_f32                                dims 1, 65, 384, 1000
  q16   crs_queries_to_f16 (padded for either slab type)   dims 1, 65, 384, 1000
  ip    crs_slab_append_space_f32, R = 2                   dims 1, 65, 384, 1024
  l2    crs_slab_append_space_f32, R = 2^-10 and 2         dims 1, 127, 383, 1023
"""
import numpy as np

import _slab_ref
import _space_build_ref

F16, I8 = 0, 1
N_ROWS = 5
CASES = ([("cos", st, dim, 0.0) for dim in (1, 65, 384, 1000) for st in (F16, I8)]
         + [("q16", st, dim, 0.0) for dim in (1, 65, 384, 1000) for st in (F16, I8)]
         + [("ip", st, dim, 2.0) for dim in (1, 65, 384, 1024) for st in (F16, I8)]
         + [("l2", st, dim, R) for dim in (1, 127, 383, 1023) for R in (2.0 ** -10, 2.0) for st in (F16, I8)])
ARRAYS = ("slab", "scales", "shadow", "row_err")


def key(kind, st, dim, R):
    return "%s_%s_d%d_R%g" % (kind, "i8" if st == I8 else "f16", dim, R)


def input_key(kind, dim, R):
    """The input rows do not depend on the slab type: one copy per (kind, dim, R); cos and q16 share theirs."""
    return "x_%s_d%d_R%g" % ("cos" if kind == "q16" else kind, dim, R)


def make_input(kind, dim, R):
    if kind in ("cos", "q16"):
        return _slab_ref.make_rows(N_ROWS, dim, seed=7 * dim + 1)[0]
    return _space_build_ref.make_space_rows(N_ROWS, dim, R, seed=7 * dim + 2)[0]


def run_case(kind, st, dim, R, x, device):
    """The case through rag._native on `device` -> {array name: numpy array} of what it wrote (fp16 as its int16 bit pattern)."""
    import torch
    from rag import _native as nat
    emb = torch.from_numpy(x).to(device)
    if kind == "q16":
        out = nat.queries_to_f16(emb, st)
        torch.cuda.synchronize()
        return {"slab": out.view(torch.int16).cpu().numpy()}
    space = {"cos": nat.SPACE_COSINE, "ip": nat.SPACE_IP, "l2": nat.SPACE_L2}[kind]
    sdim = nat.space_row_dim(dim, space)
    slab = torch.zeros((N_ROWS, nat.padded_dim(sdim, st)), dtype=torch.int8 if st == I8 else torch.float16, device=device)
    scales = torch.zeros(N_ROWS, dtype=torch.float32, device=device) if st == I8 else None
    shadow = torch.zeros((N_ROWS, sdim), dtype=torch.float32, device=device)
    row_err = torch.zeros(1, dtype=torch.float32, device=device)
    if kind == "cos":
        nat.slab_append_f32(emb, slab, 0, st, scales=scales, shadow=shadow, row_err=row_err)
    else:
        norm_scale = torch.full((1,), float(R), dtype=torch.float32, device=device)
        nat.slab_append_space_f32(emb, space, norm_scale, slab, 0, scales=scales, shadow=shadow, row_err=row_err)
    torch.cuda.synchronize()
    got = {"slab": (slab if st == I8 else slab.view(torch.int16)).cpu().numpy(), "shadow": shadow.cpu().numpy(),
           "row_err": row_err.cpu().numpy()}
    if st == I8:
        got["scales"] = scales.cpu().numpy()
    return got
