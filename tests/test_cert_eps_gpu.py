"""GPU: the certificate's eps_q (cert_query_partials / cert_query_eps, csrc/tail_steps.h) against its definition and against
what it claims to bound.

eps_q is not an output, but refine_f32_cert takes cand_scores as an input: with all k_in slots valid and in-shard and
n_rows > k_in it returns status 0 exactly when kth > t + eps_q + 2e-5 |t|, t = min(cand_scores[q]), kth = out_scores[q, k_out-1].
So cand_scores[q, :] is overwritten with one value t_q per query and t_q is bisected over the fp32 numbers (all queries at
once, one launch per step, <= 33 steps); eps_meas = kth - t* - 2e-5 |t*| at the largest certifying t*.  Only the public API is
used; the workspace's layout is never read.

  eps_q is the documented quantity:  eps_formula64 - 3 * 2^-24 <= eps_meas <= 1.0004 eps_formula64 + 3 * 2^-24
      (_slab_ref.eps_window: the kernel's three safety factors; the fp32 resolution of t and of the comparison)
  eps_q bounds reality:  eps_meas >= max over ALL rows of |slab score - fp32 score| in fp64, and >= the device's own
      |slab score - fp32 score| on its top-64 rows.

Slab, shadow and E come from the product's build, which test_slab_build_gpu.py checks against fp64.  The corpus is 2000 unit
gaussian rows; half the queries are random, half lean into one row's quantisation error (_slab_ref.cert_queries).
test_slab_ref_cpu.py shows on these inputs that the window rejects a dropped wave partial, a missing int8 fixed-point term and
the fp16 padded length on an int8 slab.  The share of eps_q that real deviations use is printed (-s) and recorded in DESIGN.md.
"""
import numpy as np
import pytest
import torch

import _slab_ref as ref
from rag import _native as nat

pytestmark = pytest.mark.gpu

F16, I8 = ref.SLAB_F16, ref.SLAB_I8
IDS = {F16: "f16", I8: "i8"}
N, NQ, K_IN, K_OUT = ref.CERT_ROWS, ref.CERT_NQ, ref.CERT_K_IN, ref.CERT_K_OUT
CASES = [(st, dim) for st in (F16, I8) for dim in ref.CERT_DIMS]


def _key(f):
    """fp32 -> an integer that orders like the float."""
    b = np.asarray(f, np.float32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7FFFFFFF))


def _unkey(k):
    bits = np.where(k >= 0, k, (-k) | 0x80000000).astype(np.uint32)
    return bits.view(np.float32)


class Case:
    def __init__(self, cuda, st, dim):
        self.cuda, self.st, self.dim = cuda, st, dim
        self.pdim = pdim = nat.padded_dim(dim, st)
        corpus = torch.from_numpy(ref.cert_corpus(dim)).to(cuda)
        self.slab = torch.empty((N, pdim), dtype=torch.int8 if st == I8 else torch.float16, device=cuda)
        self.scales = torch.empty(N, dtype=torch.float32, device=cuda) if st == I8 else None
        self.shadow = torch.empty((N, dim), dtype=torch.float32, device=cuda)
        row_err = torch.zeros(1, dtype=torch.float32, device=cuda)
        nat.slab_append_f32(corpus, self.slab, 0, st, scales=self.scales, shadow=self.shadow, row_err=row_err)
        self.E = float(row_err.item())
        self.h_slab = self.slab.cpu().numpy()
        self.h_scales = self.scales.cpu().numpy() if st == I8 else None
        self.h_shadow = self.shadow.cpu().numpy()
        assert self.E > 0 and ref.row_error64(self.h_slab, self.h_scales, self.h_shadow, dim, st).max() <= self.E
        self.h_q32 = ref.cert_queries(dim, ref.stored64(self.h_slab, self.h_scales, dim, st), self.h_shadow)
        self.q32 = torch.from_numpy(self.h_q32).to(cuda)
        self.q16 = nat.queries_to_f16(self.q32, st)
        self.h_q16 = self.q16.cpu().numpy()
        self.cand_s, self.cand_i = nat.cosine_topk(self.q16, self.slab, N, dim, K_IN, slab_type=st, scales=self.scales)
        self.ws = torch.empty(nat.exact_workspace_bytes(NQ), dtype=torch.uint8, device=cuda)
        torch.cuda.synchronize()
        ids = self.cand_i.cpu().numpy()
        assert ((ids >= 0) & (ids < N)).all() and N > K_IN          # every slot valid and in-shard: the verdict is the bound's
        self._meas = {}

    def _status(self, t):
        cs = torch.from_numpy(np.ascontiguousarray(np.repeat(t[:, None], K_IN, axis=1))).to(self.cuda)
        s, _, st = nat.refine_f32_cert(self.q32, self.q16, self.shadow, N, 0, self.cand_i, cs, K_OUT, self._row_err, self.st, self.ws)
        torch.cuda.synchronize()
        return s[:, K_OUT - 1].cpu().numpy(), st.cpu().numpy()

    def eps_meas(self, row_err):
        """Bisect t per query over the fp32 numbers in (kth - 2, kth); row_err is refine_f32_cert's row_err_max argument."""
        if row_err in self._meas:
            return self._meas[row_err]
        self._row_err = row_err
        kth, st_hi = self._status(np.zeros(NQ, np.float32))
        assert np.isfinite(kth).all()
        kth, st_hi = self._status(kth)                              # t = kth: eps_q > 0, so nothing certifies
        lo_t = (kth - np.float32(2.0)).astype(np.float32)           # eps_q < 1: everything certifies
        kth2, st_lo = self._status(lo_t)
        assert np.array_equal(kth, kth2), "the k-th fp32 score must not depend on cand_scores"
        assert (st_hi == 1).all() and (st_lo == 0).all()
        lo, hi = _key(lo_t), _key(kth)
        steps = 0
        while (hi - lo > 1).any():
            mid = (lo + hi) // 2
            _, st = self._status(_unkey(mid))
            lo = np.where(st == 0, mid, lo)
            hi = np.where(st == 0, hi, mid)
            steps += 1
            assert steps <= 33
        t = _unkey(lo).astype(np.float64)
        self._meas[row_err] = kth.astype(np.float64) - t - 2e-5 * np.abs(t)
        return self._meas[row_err]

    def formula(self, E):
        return ref.eps_formula64(self.h_q32, self.h_q16, self.dim, self.pdim, self.st == I8, E)


@pytest.fixture(scope="module")
def case(cuda):
    memo = {}

    def get(st, dim):
        if (st, dim) not in memo:
            memo[(st, dim)] = Case(cuda, st, dim)
        return memo[(st, dim)]
    return get


def _in_window(meas, formula, what):
    lo, hi = ref.eps_window(formula)
    bad = np.flatnonzero((meas < lo) | (meas > hi))
    assert bad.size == 0, f"{what}: query {bad[0]}: eps_meas {meas[bad[0]]!r} outside [{lo[bad[0]]!r}, {hi[bad[0]]!r}]"


@pytest.mark.parametrize("st,dim", CASES, ids=lambda v: IDS.get(v, str(v)) if v in (F16, I8) else str(v))
def test_eps_is_the_documented_quantity(case, st, dim):
    c = case(st, dim)
    _in_window(c.eps_meas(c.E), c.formula(c.E), "measured E")
    # row_err_max = -1: the store did not track E, the analytic bound takes its place
    bound = nat.exact_row_error_bound(dim, st)
    assert bound >= c.E
    _in_window(c.eps_meas(-1.0), c.formula(bound), "analytic E")


@pytest.mark.parametrize("st", [F16, I8], ids=IDS.get)
def test_eps_moves_with_E_by_the_formulas_amount(case, st):
    c = case(st, 384)
    E2 = float(np.float32(2.0 * c.E))
    m1, m2 = c.eps_meas(c.E), c.eps_meas(E2)
    _in_window(m2, c.formula(E2), "E doubled")
    # eps_q is affine in E with slope dq 1.0001^2 + |q| 1.0002: the step is within [1, 1.0003] of the formula's, and each of the two
    # measurements resolves to 3 * 2^-24
    d = c.formula(E2) - c.formula(c.E)
    assert (d > 100 * ref.U).all()
    assert (m2 - m1 >= d - 6 * ref.U).all() and (m2 - m1 <= 1.0004 * d + 6 * ref.U).all()


@pytest.mark.parametrize("st,dim", CASES, ids=lambda v: IDS.get(v, str(v)) if v in (F16, I8) else str(v))
def test_eps_bounds_the_slab_scores_deviation(case, st, dim):
    c = case(st, dim)
    eps = c.eps_meas(c.E)
    # fp64, every row of the shard
    dev = ref.slab_deviation64(c.h_q32, c.h_q16, c.h_slab, c.h_scales, c.h_shadow, st)
    assert (dev <= eps).all(), f"a row deviates by {dev.max()!r}, more than eps_q allows"
    # the device's own scores on its top-64 rows: slab score against the fp32 score of the same row
    s_slab, ids = nat.cosine_topk(c.q16, c.slab, N, dim, 64, slab_type=st, scales=c.scales)
    s_32 = nat.score_rows_f32(c.q32, c.shadow, N, 0, ids)
    torch.cuda.synchronize()
    assert (ids.cpu().numpy() >= 0).all()
    dev_d = np.abs(s_slab.cpu().numpy().astype(np.float64) - s_32.cpu().numpy().astype(np.float64)).max(axis=1)
    assert (dev_d <= eps).all()
    half = NQ // 2
    print(f"\ncert_eps {IDS[st]} dim {dim}: E {c.E:.4e}  eps_q {eps.min():.4e}..{eps.max():.4e}  max deviation/eps_q: "
          f"random {(dev[:half] / eps[:half]).max():.3f}  adversarial {(dev[half:] / eps[half:]).max():.3f}  device top-64 {(dev_d / eps).max():.3f}")
