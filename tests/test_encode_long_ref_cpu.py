"""The Python reference of the long-word tests (encode_long_ref.py) against the oracle encoder
(oracle/encode_oracle.c) on words the oracle takes (at most 1024 bytes): identical ids.  This is
the chain of trust of test_gpu_encode_long.py, whose words the oracle refuses."""
import os

import numpy as np
import pytest

import corpora
from conftest import GOLDEN
from encode_long_ref import TABLES, ref_encode
from encode_ref import model_merges, oracle_encode

GOLDEN_MODEL = "c1_ascii10m_v8192"


def golden_merges():
    with open(os.path.join(GOLDEN, GOLDEN_MODEL, "model.bin"), "rb") as f:
        return model_merges(f.read())


def golden_text(tmp_path, nbytes=24000):
    """The first bytes of the golden model's own corpus generator (same seed and script)."""
    path = str(tmp_path / "c.txt")
    corpora.gen_synthetic(path, nbytes, 1, "ascii")
    with open(path, "rb") as f:
        return f.read()


def test_reference_equals_oracle_on_golden_corpus(tmp_path):
    merges, text = golden_merges(), golden_text(tmp_path)
    assert len(text.split()) >= 2000
    got = ref_encode(merges, None, text)
    assert np.array_equal(got, oracle_encode(merges, None, text))
    assert got.size < len(text.replace(b" ", b"").replace(b"\n", b"")) // 2  # the merges do apply


HAND_TEXTS = [
    b"a" * 1024 + b" " + b"a" * 1023 + b"\n" + b"a" * 7 + b"\t" + b"a",
    b"b".join(b"a" * k for k in range(1, 10)) + b" " + b"ab" * 100 + b"\r\n" + b"aabaaabaaaab",
    b"abcd" * 256 + b" abcd abc ab a dcba " + b"abcdabc" * 50 + b"\n" + b"xyxxyx" * 20 + b" abcdxyabcd",
    b"",
    b" \n\t",
]


@pytest.mark.parametrize("table", sorted(TABLES))
def test_reference_equals_oracle_on_hand_tables(table):
    for text in HAND_TEXTS:
        assert np.array_equal(ref_encode(TABLES[table], None, text), oracle_encode(TABLES[table], None, text)), \
            (table, text[:40])


def test_reference_byte_map_and_unk():
    bm = np.arange(256, dtype=np.int32)
    bm[ord("b")] = -1  # a dropped byte never merges
    text = b"aabaab abab " + b"a" * 300 + b"b" + b"a" * 301
    for table in ("aa", "aa_aaaa", "local_min"):
        assert np.array_equal(ref_encode(TABLES[table], bm, text), oracle_encode(TABLES[table], bm, text))


def test_local_minimum_counter_example():
    """abcd under 0:(a,b)->X, 1:(X,c)->Y, 5:(c,d)->Z is Y d; merging every local minimum would give X Z."""
    ids = ref_encode(TABLES["local_min"], None, b"abcd")
    assert ids.tolist() == [257, ord("d")]
    assert ref_encode(TABLES["local_min_2"], None, b"abcd").tolist() == [257, ord("d")]
