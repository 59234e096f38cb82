"""The condition that keeps the GPU tests of chained launches from passing vacuously, proved on the
CPU from the host logic alone: with `chain` = 2 or 8 the engine really sends chains to the backend
on the corpora those tests use -- launches of >= 2 and of 8 merges, tails confirmed, tails rejected
with >= 2 merges to undo at once -- and the outputs are still the reference's.

The engine's choices (how long a chain, which guess is confirmed) depend on the selector alone, which
sees the same pair counts in both layouts; the shapes are run in both, the larger goldens in `types`.

What cannot form a chain, and is left out of the chain matrix's "chains formed" assertions:
* the degenerate shapes: at most 7 merges, and `remaining` (vocab target or batch end) cuts every
  chain but one_run's single launch of 2;
* `chain` = 2 never undoes two merges at once (a tail of one), so the >= 2 undo is asserted for 8 only;
* bpe_merge_batch(1): `remaining` = 1 cuts every chain to 1, so a trainer stepped one merge at a time
  never chains.  The stepped tests therefore step by 8."""
import pytest

import hostharness
import shape_corpora as sc
from conftest import golden_cases

CHAIN_SHAPES = [n for n in sc.TRAINER_SHAPES if n not in sc.DEGENERATE]
API_CASES = [n for n in golden_cases() if not n.startswith("cli_")]
DEEP = [n for n in API_CASES if "v32000" in n or "v64000" in n]
STREAM_GOLDENS = ["c1_ascii10m_v8192", "ascii1m_v3000_mpf2", "adv_unk0", "adv_unkm1", "ascii1m_unk7_cov09", "small_v300"]


@pytest.fixture(scope="module")
def hh():
    return hostharness.load()


@pytest.fixture(scope="module")
def shape_corpus(tmp_path_factory):
    import corpora
    root, made = tmp_path_factory.mktemp("shapes"), {}

    def get(name):
        if name not in made:
            case, path = sc.load_fixture(name), str(root / f"{name}.txt")
            sc.build(name, path)
            assert corpora.md5_file(path) == case["corpus"]["md5"], f"generator drift for {name}"
            made[name] = (case, path)
        return made[name]
    return get


def _train(hh, case, corpus, layout, chain, tmp_path):
    h = hostharness.open_case(hh, corpus, case["config"], layout)
    try:
        hh.hh_set_chain(h, chain)
        trace, model, vocab = (str(tmp_path / n) for n in ("t.txt", "h.model", "h.vocab"))
        merges = hh.hh_train(h, trace.encode())
        hh.hh_save(h, model.encode(), vocab.encode(), 1)
        got = (merges, open(trace).read(), open(model, "rb").read(), open(vocab, "rb").read())
        return got, hostharness.chain_stats(hh, h)
    finally:
        hh.hh_close(h)


def _check_chains(cs, chain):
    assert cs["launches_ge2"] > 0 and cs["tails_confirmed"] > 0 and cs["max_len"] == chain, cs
    if chain == 8:
        assert cs["launches_8"] > 0 and cs["undos_ge2"] > 0 and cs["max_undo"] >= 2, cs
    else:
        assert cs["max_undo"] == 1 and cs["undos_ge2"] == 0, cs   # a tail of one


@pytest.mark.parametrize("chain", [2, 8])
@pytest.mark.parametrize("layout", ["types", "stream"])
@pytest.mark.parametrize("name", sc.TRAINER_SHAPES)
def test_shapes_form_chains(name, layout, chain, hh, shape_corpus, tmp_path):
    """Per corpus: every non-degenerate trainer shape launches chains of the full length, confirms
    tails and (chain 8) undoes >= 2 merges at once; the degenerate ones run too and never chain
    beyond one_run's one launch of 2."""
    case, corpus = shape_corpus(name)
    got, cs = _train(hh, case, corpus, layout, chain, tmp_path)
    assert got == (case["merges"], case["trace"], case["model_bytes"], case["vocab_bytes"])
    if name in CHAIN_SHAPES:
        _check_chains(cs, chain)
    else:
        assert cs["launches_8"] == 0 and cs["undos_ge2"] == 0 and cs["max_len"] <= 2, cs
        assert (cs["launches_ge2"], cs["tails_confirmed"]) == ((1, 1) if name == "one_run" else (0, 0)), cs


@pytest.mark.parametrize("name,chain", [(n, k) for n in API_CASES if n not in DEEP for k in (2, 8)] +
                         [pytest.param("mixed24m_v64000_cov9995_mpf2", 8, marks=pytest.mark.slow)])
def test_goldens_form_chains(name, chain, hh, case_corpus, tmp_path):
    """Per golden that the GPU parity test chains (every API golden that is not deep, the stream
    layout's list among them, and the one deep run it takes)."""
    case, corpus = case_corpus(name)
    got, cs = _train(hh, case, corpus, "types", chain, tmp_path)
    assert got == (case["merges"], case["trace"], case["model_bytes"], case["vocab_bytes"])
    if case["merges"] >= 50:
        _check_chains(cs, chain)


def test_stream_golden_list_is_covered():
    assert set(STREAM_GOLDENS) <= set(API_CASES) - set(DEEP)


@pytest.mark.parametrize("layout", ["types", "stream"])
@pytest.mark.parametrize("name", ["tile_edge", "chunk_edge"])
def test_stepped_training_chains_only_in_batches(name, layout, hh, shape_corpus):
    """The stepped long-tile undo test's protocol: 56 merges in batches of 8 under chain 8 launch
    full chains and undo >= 2 merges at once; the same merges one per batch never chain."""
    case, corpus = shape_corpus(name)
    for batch, chained in ((1, False), (8, True)):
        h = hostharness.open_case(hh, corpus, case["config"], layout)
        try:
            hh.hh_set_chain(h, 8)
            hh.hh_init(h)
            done = 0
            while done < 56:
                k = hh.hh_merge_batch(h, batch)
                assert k == batch
                done += k
            cs = hostharness.chain_stats(hh, h)
        finally:
            hh.hh_close(h)
        if chained:
            assert cs["launches_8"] > 0 and cs["undos_ge2"] > 0 and cs["tails_confirmed"] > 0, cs
        else:
            assert cs["max_len"] == 1 and cs["launches"] == 56 and cs["max_undo"] == 0, cs


@pytest.mark.parametrize("chain", [2, 8])
def test_lockstep_chunks_form_chains(chain, hh, tmp_path):
    """The GPU lockstep's protocol on its medium corpus: chunks of 1, 2, 7, 8, 9, 64 and 300 merges,
    six times over, cut chains short at their ends and still launch full ones."""
    import corpora
    corpus = str(tmp_path / "m.txt")
    corpora.gen_synthetic(corpus, 12_000_000, 31, "mixed")
    cfg = dict(vocab_size=6000, unk_id=0, character_coverage=0.9995, min_pair_freq=20)
    h = hostharness.open_case(hh, corpus, cfg, "types")
    try:
        hh.hh_set_chain(h, chain)
        hh.hh_init(h)
        for chunk in [1, 2, 7, 8, 9, 64, 300] * 6:
            assert hh.hh_merge_batch(h, chunk) == chunk
        cs = hostharness.chain_stats(hh, h)
    finally:
        hh.hh_close(h)
    _check_chains(cs, chain)


def test_chain_index_leaves_room_for_the_tile(hh):
    """Device::max_chain()'s bound: a matched-tile entry is tile | chain index << kChainShift, so
    chains run only while every tile index stays below 2^kChainShift, and 8 chain indices fit above
    it.  (The predicate alone: that max_chain() consults it is not reachable without a device.)"""
    shift = hh.hh_device_chain_shift()
    assert shift + 3 <= 32
    assert hh.hh_device_chain_fits((1 << shift) - 1) == 1
    assert hh.hh_device_chain_fits(1 << shift) == 0
    assert hh.hh_device_chain_fits(1 << 32) == 0
    assert hh.hh_device_chain_fits(0) == 1
