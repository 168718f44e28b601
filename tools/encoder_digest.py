#!/usr/bin/env python3
"""SHA-256 of every output array of the encoder on the suites' seeded cases (needs a GPU).

  python tools/encoder_digest.py > digest.txt

Run it against two builds (CRS_LIB_PATH, or two checkouts) and diff the outputs: a refactor of the attention or embedding
kernels (csrc/enc_attn.hip, csrc/enc_misc.hip) must leave every line as it was.  The GPU suites compare with fp64 inside
a tolerance and cannot see a changed rounding point; this does.  Covered: every case of tests/_encoder_cases.ALL_CASES
through the default dispatch; every case of tests/_mpnet_cases.CASES (relative bias), default and small_lds selection;
the cases of tests/_crossenc_cases.py with their type ids and with type_ids=None; the forwards of tests/_nomic_cases.py (rotary)
and tests/_modernbert_cases.py (rotary, windowed); every attention kernel on its own: each case of tests/_attn_cases.CASES
at its route, and attention_window_f16 at the shapes, lens and seeds of tests/test_modernbert_gpu.py's window test.  Every
output is digested whole, padding rows included: the window kernel's zero rows and finite padding rows are its behaviour."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)
import _attn_cases as ac  # noqa: E402
import _attn_ref as ar  # noqa: E402
import _crossenc_cases as cc  # noqa: E402
import _encoder_cases as ec  # noqa: E402
import _modernbert_cases as mb  # noqa: E402
import _mpnet_cases as mc  # noqa: E402
import _nomic_cases as nc  # noqa: E402
from rag import _encoder as enc_api  # noqa: E402
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


def pooled_forwards(case, enc, ids, lens):
    """final hidden states, mean and CLS embeddings (the rotary models)"""
    enc.desc.pooling = 0
    mean, hidden = enc.forward(ids, lens, return_hidden=True)
    enc.desc.pooling = 1
    cls = enc.forward(ids, lens)
    emit(case, hidden=hidden, mean=mean, cls=cls)


def attention_alone():
    """the attention entry points on their own, into a buffer preset to 7.0 so that an unwritten row shows"""
    for c in ac.CASES:
        inp = ac.case_inputs(c)
        lens = torch.tensor(c.lens, dtype=torch.int32, device=DEV)
        ctx = torch.full((c.batch * c.seq, c.heads * c.hd), 7.0, dtype=torch.float16, device=DEV)
        if c.form == "fused":
            x16, w, bq = (torch.from_numpy(a).to(DEV) for a in inp)
            enc_api.qkv_attn_f16(x16, w, bq, lens, ctx, c.batch, c.seq, c.heads)
        else:
            bias = torch.from_numpy(inp[1]).to(DEV) if c.span else None
            enc_api.attention_f16(torch.from_numpy(inp[0]).to(DEV), lens, ctx, c.batch, c.seq, c.heads, bias, c.route)
        emit("attn " + ac.attn_id(c), ctx=ctx)
    for hd, heads in ((16, 4), (32, 3), (64, 2)):
        for window in (1, 8, 64, 200):
            for seq in (16, 80, 144, 200):
                lens = [seq, 5, max(1, (seq * 5) // 8)]
                qkv = ar.make_inputs(len(lens), seq, heads, hd, lens, seed=hd * 100000 + window * 1000 + seq, peaked=True)
                ctx = torch.full((len(lens) * seq, hd * heads), 7.0, dtype=torch.float16, device=DEV)
                enc_api.attention_window_f16(torch.from_numpy(qkv).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), ctx,
                                             len(lens), seq, heads, window)
                emit(f"window hd{hd} W{window} s{seq}", ctx=ctx)


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
    for key, cfg, seed, batch, seq in nc.CASES:
        ids, mask = nc.synth_tokens(cfg, batch, seq, seed + 1)
        pooled_forwards("nomic " + key, HipEncoder(nc.model_shape(cfg), nc.make_weights(cfg, seed), device=DEV), ids, mask.sum(1).astype(np.int32))
    for key, cfg, seed, lens, seq in mb.CASES:
        ids, mask = mb.synth_tokens(cfg, lens, seq, seed + 1)
        pooled_forwards("modernbert " + key, HipEncoder(mb.model_shape(cfg), mb.make_weights(cfg, seed), device=DEV), ids, mask.sum(1).astype(np.int32))
    attention_alone()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
