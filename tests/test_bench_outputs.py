"""bench.py --dump-outputs: what the timed path computed in its last step, as .npy files (CPU: the writer on a made-up result;
GPU: two plain runs with the same arguments write the same arrays)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from jasper_amd.table import FIXREC_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("histogram", "threshold", "count_totals", "qv_counters", "fix_records", "fix_patches", "polished_lengths",
         "polished_text_sample", "polished_block_sums")


class _Result:
    def __init__(self, seqs, raw, aux, qv):
        self._seqs, self._raw, self.aux, self.qv = seqs, raw, aux, qv

    def seq_view(self, i):
        return memoryview(self._seqs[i])


def _records(rows):
    raw = np.zeros(len(rows), dtype=FIXREC_DTYPE)
    for i, (chunk, pass_, seqno, kind, index, rep, aux_off, aux_len) in enumerate(rows):
        raw[i] = (index, chunk, seqno, pass_, ord(kind), ord("A"), ord("C"), rep, aux_off, aux_len)
    return raw


def test_dump_outputs_writes_the_last_step(tmp_path):
    seqs = [b"ACGT" * 3000, b"", b"TTGCA" * 1001]
    # out of (chunk, pass, seqno) order on purpose; the 'x' record of chunk 2 references "GG" (patch) + "ACG" (original)
    raw = _records([(2, 0, 1, "x", 40, 3, 2, 2), (0, 1, 0, "s", 7, 1, 0, 0), (0, 0, 5, "i", 9, 0, 0, 0), (0, 0, 2, "d", 3, 1, 0, 0)])
    aux = [b"", b"", b"..GGACG"]
    res = _Result(seqs, raw, aux, (3, 100, 1, 100))
    T = dict(rows=[(1, 50), (2, 7), (9, 1)], thr=2, distinct=58, occurrences=73)
    bench.dump_outputs(str(tmp_path), res, T, len(seqs), 0, 1)
    got = {n: np.load(tmp_path / (n + ".npy")) for n in NAMES}
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in NAMES)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["histogram"].tolist() == [[1, 50], [2, 7], [9, 1]]
    assert got["threshold"].tolist() == [2] and got["count_totals"].tolist() == [58, 73] and got["qv_counters"].tolist() == [3, 100, 1, 100]
    assert got["fix_records"][:, :3].tolist() == [[0, 0, 2], [0, 0, 5], [0, 1, 0], [2, 0, 1]]       # sorted by (chunk, pass, seqno)
    assert got["fix_records"][:, 3].tolist() == [ord(c) for c in "disx"]
    assert bytes(got["fix_patches"].astype(np.uint8)) == b"GGACG"
    text = b"".join(seqs)
    assert got["polished_lengths"].tolist() == [len(s) for s in seqs]
    assert bytes(got["polished_text_sample"].astype(np.uint8)) == text       # (shorter than the sample: all of it)
    big = _Result([b"ACGTN" * (bench.DUMP_TEXT_SAMPLE // 4)], raw[:0], [b""], (0, 0, 0, 0))
    bench.dump_outputs(str(tmp_path / "big"), big, T, 1, 0, 1)
    sample = np.load(tmp_path / "big" / "polished_text_sample.npy")
    assert len(sample) == bench.DUMP_TEXT_SAMPLE and set(sample.astype(np.uint8).tobytes()) == set(b"ACGTN")
    assert np.load(tmp_path / "big" / "fix_records.npy").shape == (0, 8) and len(np.load(tmp_path / "big" / "fix_patches.npy")) == 0
    sums = got["polished_block_sums"]
    assert len(sums) == -(-len(text) // bench.DUMP_BLOCK)
    assert sums[-1] == sum(b * (i + 1) for i, b in enumerate(text[(len(sums) - 1) * bench.DUMP_BLOCK:]))
    assert sum(a.nbytes for a in got.values()) < 64 << 20
    # the same result gives the same files; one other base gives other block sums
    bench.dump_outputs(str(tmp_path / "again"), res, T, len(seqs), 0, 1)
    assert all(np.array_equal(got[n], np.load(tmp_path / "again" / (n + ".npy"))) for n in NAMES)
    seqs[0] = b"C" + seqs[0][1:]
    bench.dump_outputs(str(tmp_path / "other"), res, T, len(seqs), 0, 1)
    assert not np.array_equal(sums, np.load(tmp_path / "other" / "polished_block_sums.npy"))


@pytest.mark.gpu
def test_plain_bench_runs_write_the_same_outputs(hip, tmp_path):
    """two plain `bench.py` runs with the same arguments: the timed steps asked for, ms_per_step, none of the --full legs, and
    the same arrays in --dump-outputs"""
    outs = []
    for run in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--genome-mb", "2",
                            "--dump-outputs", str(tmp_path / run)], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        outs.append(json.loads(lines[0]))
    for out in outs:
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "Mbp/s"
        assert not {"cpu_baseline", "e2e_cli", "polish_host_io_ms"} & set(out)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in NAMES) == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) < 64 << 20
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    h = np.load(tmp_path / "a" / "histogram.npy")
    assert len(h) and np.all(np.diff(h[:, 0]) > 0) and np.all(h[:, 1] > 0)
    assert np.load(tmp_path / "a" / "count_totals.npy")[0] == outs[0]["config"]["distinct_kmers"]
    assert np.load(tmp_path / "a" / "threshold.npy").tolist() == [outs[0]["config"]["threshold"]]
    assert np.load(tmp_path / "a" / "qv_counters.npy").tolist() == outs[0]["qv_counters"]
    assert len(np.load(tmp_path / "a" / "fix_records.npy")) == outs[0]["fix_records"]
