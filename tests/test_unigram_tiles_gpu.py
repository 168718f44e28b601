"""GPU: crs_unigram_encode (csrc/unigram.hip) across tile boundaries, for every value of its option bits.  One pipeline per
option set (tests/_unigram_cases.OPTION_SETS); the boundary sweep at a row that holds every id and at rows whose budget ends
inside the first tile; 300 seeded texts of 1 to 3.5 KB; lens, every id, the padding and the flags against
`UnigramTokenizer.encode` and `rag._unigram.emulate_encode`, as integers.  tests/test_unigram_tiles_cpu.py holds the same texts
to the `tokenizers` library."""
import json
import os

import numpy as np
import pytest

import _unigram_cases as uc
import _xlmr_cases as xc

pytestmark = pytest.mark.gpu

NAMES = tuple(uc.OPTION_SETS)
_DT, _CASES, _EMU_NONE = {}, {}, {}


def device_side(name, cuda):
    """(restatement, spec, table, vocabulary, device tokeniser) of an option set, built once for the module."""
    if name == "spm":
        pytest.importorskip("tokenizers")
    tok, spec, table, vocab, opts = uc.side(name)
    if name not in _DT:
        from rag import _unigram as ug
        _DT[name] = ug.UnigramDeviceTokenizer(tok, cuda)
        assert _DT[name].opts == opts == uc.OPTION_SETS[name] and _DT[name].table is table
    return tok, spec, table, vocab, _DT[name]


def cases(kind, table):
    """[(name, text)] of the sweep, or of the random long texts over the table's non-FALLBACK code points; built once."""
    from rag import _native as nat
    key = (kind, id(table))
    if key not in _CASES:
        if kind == "sweep":
            _CASES[key] = tuple(uc.boundary_sweep(nat.UNIGRAM_TILE_BYTES, nat.UNIGRAM_MAX_WORD))
        else:
            allowed = np.nonzero(~table.fallback_mask())[0]
            _CASES[key] = tuple((f"random-{i}", t) for i, t in enumerate(uc.random_long_texts(300, 51, allowed)))
    return _CASES[key]


def emulation_flags(name, kind, side):
    """The names of the texts the emulation returns None for (its answer does not depend on the row's width); once per set."""
    from rag import _unigram as ug
    tok, spec, table, vocab, dt = side
    if (name, kind) not in _EMU_NONE:
        _EMU_NONE[name, kind] = {n for n, t in cases(kind, table) if ug.emulate_encode(t, table, vocab, spec, 16) is None}
    return _EMU_NONE[name, kind]


def run(dt, texts, width):
    import torch
    ids, lens, flags, host = dt.encode(texts, width)
    torch.cuda.synchronize()
    assert host == []
    return ids.cpu().numpy(), lens.cpu().numpy(), flags.cpu().numpy()


def check(name, cuda, kind, width, want_flagged):
    from rag import _native as nat
    assert nat.UNIGRAM_TILE_BYTES == 1024 and nat.UNIGRAM_MAX_WORD == 128
    side = device_side(name, cuda)
    tok, spec, table, vocab, dt = side
    names, texts = [n for n, _ in cases(kind, table)], [t for _, t in cases(kind, table)]
    # nothing is skipped silently: before the launch, the emulation flags the named cases over the cap and nothing else
    emu_none = emulation_flags(name, kind, side)
    assert emu_none == want_flagged(names, table), (name, kind)
    ids, lens, flags = run(dt, texts, width)
    assert ids.shape == (len(texts), width) and ids.dtype == np.int32
    bad = []
    for r, (case, text) in enumerate(zip(names, texts)):
        if case in emu_none:
            # a text the emulation flags may pass unflagged only when the row filled up before the kernel read that far
            if flags[r] == 1:
                continue
            if not (flags[r] == 0 and lens[r] == width):
                bad.append((case, "not flagged", int(flags[r]), int(lens[r])))
                continue
        elif flags[r] != 0:
            bad.append((case, "flagged", int(flags[r])))
            continue
        want = tok.encode(text, width)
        if lens[r] != len(want):
            bad.append((case, "lens", int(lens[r]), len(want)))
        elif ids[r, : lens[r]].tolist() != want:
            k = int(np.nonzero(ids[r, : lens[r]] != np.asarray(want))[0][0])
            bad.append((case, "id", k, ids[r, k: k + 4].tolist(), want[k: k + 4]))
        elif not (ids[r, lens[r]:] == tok.pad_id).all():
            bad.append((case, "padding"))
    assert not bad, (name, kind, width, len(bad), bad[:12])
    return flags, names


def sweep_flagged(names, table):
    from rag import _unigram as ug
    return uc.sweep_flagged(names, table.lookup(ord(uc.DROPPED))[0] == ug.DROP)


@pytest.mark.parametrize("width", [4096, 16, 64])
@pytest.mark.parametrize("name", NAMES)
def test_sweep_equals_the_restatement(cuda, name, width):
    """4096 holds every id of every text; 16 and 64 end the row inside the first tile, and the kernel must stop there."""
    flags, names = check(name, cuda, "sweep", width, sweep_flagged)
    if width == 4096:          # the row never fills: every text over the cap is flagged, the word at the cap is not
        assert {n for n, f in zip(names, flags) if f} == sweep_flagged(names, device_side(name, cuda)[2])
        assert all(not flags[names.index(f"cap-0@{b}-{j}")] and flags[names.index(f"overcap-1@{b}-{j}")] == 1
                   for b in (1024, 2048) for j in (1, 2, 3))


@pytest.mark.parametrize("name", NAMES)
def test_random_long_texts_equal_the_restatement(cuda, name):
    flags, _ = check(name, cuda, "random", 2048, lambda names, table: set())
    assert not flags.any()


def test_two_launches_give_identical_bytes(cuda):
    tok, spec, table, vocab, dt = device_side("alone-always.none", cuda)
    texts = [t for _, t in cases("sweep", table)]
    a, b = run(dt, texts, 4096), run(dt, texts, 4096)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


# ---- EmbeddingModel ------------------------------------------------------------------------------------------------------------------
def _forward_blocks(model, texts):
    """[(ids, lens) of every HipEncoder.forward call] of one embed_device."""
    import torch
    calls = []
    real = model.model.forward

    def forward(ids, lens, *args, **kwargs):
        as_np = lambda x: x.detach().cpu().numpy().copy() if isinstance(x, torch.Tensor) else np.array(x)   # noqa: E731
        calls.append((as_np(ids).astype(np.int32), as_np(lens).astype(np.int32)))
        return real(ids, lens, *args, **kwargs)

    model.model.forward = forward
    try:
        model.embed_device(texts)
        torch.cuda.synchronize()
        return calls
    finally:
        model.model.forward = real


def test_embedding_model_metaspace_alone_device_tokens_equal_host_tokens(cuda, tmp_path, monkeypatch):
    """A written XLM-R directory whose tokenizer.json is Metaspace alone with no Replace (SINGLE_META without COLLAPSE): the
    (ids, lens) block of every forward call under tokenize 'device' is the one under 'host', on texts of the sweep."""
    from rag import _native as nat
    from rag.embedding import EmbeddingModel
    monkeypatch.setenv("CRS_TOKENIZER", "python")
    src = str(tmp_path / "tokenizer_src.json")
    with open(src, "w", encoding="utf-8") as fh:
        json.dump(uc.config("alone-always.none"), fh)
    d = str(tmp_path / "m")
    xc.write_xlmr_dir(d, src, seed=9, vocab_size=len(uc.vocab()))
    assert os.path.exists(os.path.join(d, "tokenizer.json"))
    sweep = uc.boundary_sweep(nat.UNIGRAM_TILE_BYTES, nat.UNIGRAM_MAX_WORD)
    texts = [t for n, t in sweep if n.startswith(("sp3@", "sp7@", "overcap-", "cap-0@"))] + [t for _, t in sweep[-4:]]
    assert 40 <= len(texts) <= 70
    host = EmbeddingModel({"model_name": d, "batch_size": 32, "tokenize": "host"})
    device = EmbeddingModel({"model_name": d, "batch_size": 32, "tokenize": "device"})
    calls_h, calls_d = _forward_blocks(host, texts), _forward_blocks(device, texts)
    assert type(device._device_tokenizer).__name__ == "UnigramDeviceTokenizer"
    assert device._device_tokenizer.opts == nat.UNIGRAM_SINGLE_META
    assert len(calls_d) == len(calls_h) == -(-len(texts) // 32)
    for b, ((ids_h, lens_h), (ids_d, lens_d)) in enumerate(zip(calls_h, calls_d)):
        assert ids_h.shape == ids_d.shape, (b, ids_h.shape, ids_d.shape)
        assert np.array_equal(lens_h, lens_d), b
        assert np.array_equal(ids_h, ids_d), b
