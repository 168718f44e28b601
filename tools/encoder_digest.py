#!/usr/bin/env python3
"""SHA-256 of every output array of the encoder on the suites' seeded cases (needs a GPU).

  python tools/encoder_digest.py > digest.txt

Run it against two builds (CRS_LIB_PATH, or two checkouts) and diff the outputs: a refactor of the attention or embedding
kernels (csrc/enc_attn.hip, csrc/enc_misc.hip) must leave every line as it was.  The GPU suites compare with fp64 inside
a tolerance and cannot see a changed rounding point; this does.  Covered: every case of tests/_encoder_cases.ALL_CASES
through the default dispatch; every case of tests/_mpnet_cases.CASES (relative bias), default and small_lds selection;
the cases of tests/_crossenc_cases.py with their type ids and with type_ids=None."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)
import _crossenc_cases as cc  # noqa: E402
import _encoder_cases as ec  # noqa: E402
import _mpnet_cases as mc  # noqa: E402
from rag import _native as nat  # noqa: E402
from rag._encoder import HipEncoder  # noqa: E402

DEV = torch.device("cuda:0")


def emit(case, **arrays):
    for name, t in arrays.items():
        a = np.ascontiguousarray(t.detach().cpu().numpy())
        print(f"{case:34s} {name:8s} {a.dtype.str} {list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


def forwards(case, enc, ids, lens, small_lds=False):
    """final hidden states, mean and CLS embeddings, the fp16 query block"""
    enc.desc.pooling = 0
    mean, hidden = enc.forward(ids, lens, return_hidden=True, small_lds=small_lds)
    q16 = torch.zeros((ids.shape[0], nat.padded_dim(enc.shape.hidden)), dtype=torch.float16, device=DEV)
    enc.forward(ids, lens, q16_out=q16, small_lds=small_lds)
    enc.desc.pooling = 1
    cls = enc.forward(ids, lens, small_lds=small_lds)
    emit(case, hidden=hidden, mean=mean, cls=cls, q16=q16)


def main():
    nat.require_gpu()
    torch.cuda.set_device(DEV)
    for case in ec.ALL_CASES:
        ids, _, lens = ec.case_inputs(case)
        forwards("enc " + case.name, ec.hip_encoder(case, DEV), ids, lens)
    for key, cfg, seed, batch, seq in mc.CASES:
        enc = HipEncoder(mc.model_shape(cfg), mc.make_weights(cfg, seed), device=DEV)
        ids, mask = mc.synth_tokens(cfg, batch, seq, seed + 1000)
        lens = mask.sum(1).astype(np.int32)
        for small in (False, True):
            forwards(f"mpnet {key}{' small_lds' if small else ''}", enc, ids, lens, small)
    for key, cfg, seed, batch, seq in cc.CASES:
        enc = HipEncoder(cc.model_shape(cfg), cc.make_weights(cfg, seed), device=DEV)
        ids, types, mask = cc.synth_pairs(cfg, batch, seq, seed + 1000)
        lens = mask.sum(1).astype(np.int32)
        for what, ty in (("types", types), ("no types", None)):
            scores, pooled, hidden = enc.score_pairs(ids, ty, lens, return_pooled=True, return_hidden=True)
            emit(f"pairs {key} {what}", scores=scores, pooled=pooled, hidden=hidden)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
