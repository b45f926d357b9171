"""CPU: the host side of `python -m jasper_amd.triobin --reader device` -- blocks and the carried tail, names, the second pass of
--write-reads that routes by remembered record starts, the fallback that words a malformed record, the flag.  The GPU's part
(KmerTable.read_bins_text) is replaced here by the restatements (tests/readtext_ref.py, tests/readbins_ref.py), as test_triobin_host.py
replaces the counter; tests/test_gpu_cli_triobin_reader.py runs the real one."""
import os
import types

import numpy as np
import pytest

import readbins_ref as ref
import readtext_ref as rt
import test_triobin_host as th


def fake_count_text(calls=None):
    def count_text(buf, eof, fmt):
        assert buf.dtype == np.uint8 and fmt in ("fastq", "fasta")
        if calls is not None:
            calls.append((len(buf), bool(eof)))
        r = types.SimpleNamespace(malformed=False, bad_record=-1, seconds=0.0, index_seconds=0.0)
        try:
            used, rec_start, head_end, lens, seq = rt.parse(buf.tobytes(), eof, fmt)
        except rt.Bad as e:
            r.malformed, r.bad_record, r.used, r.n_records = True, e.record, 0, 0
            return r
        m, p = ref.read_counts(rt.reads_of(lens, seq), th.K, th.MD, th.PD, 1, 1)
        r.used, r.n_records = used, len(lens)
        r.rec_start, r.head_end, r.lens = np.array(rec_start, dtype=np.int64), np.array(head_end, dtype=np.int64), np.array(lens, dtype=np.int64)
        r.mat, r.pat = np.array(m, dtype=np.uint32), np.array(p, dtype=np.uint32)
        return r
    return count_text


def never(text, offs):
    raise AssertionError("the device reader does not call the batch counter")


def test_device_reader_writes_what_the_host_reader_writes(tmp_path, monkeypatch):
    from jasper_amd import triobin
    files = th.write_formats(tmp_path)
    paths = [str(tmp_path / fn) for fn in files]
    host = str(tmp_path / "host")
    triobin.bin_files(paths, host, th.ref_counter(), th.M_TOTAL, th.P_TOTAL, per_read=True, write_reads=True)
    outs = sorted(fn[len("host"):] for fn in os.listdir(tmp_path) if fn.startswith("host."))
    assert len(outs) == 2 + 3 * len(paths)
    for chunk in (None, 64, 7, 1):                      # whole files, and blocks that cut every record and every line
        if chunk is None:
            monkeypatch.delenv("JASPER_TRIOBIN_CHUNK", raising=False)
        else:
            monkeypatch.setenv("JASPER_TRIOBIN_CHUNK", str(chunk))
        monkeypatch.setattr(triobin, "CHUNK", 16 << 20 if chunk is None else 5 * chunk + 3)      # (the second pass's blocks)
        calls = []
        prefix = str(tmp_path / ("dev%s" % chunk))
        per_bin, _ = triobin.bin_files(paths, prefix, never, th.M_TOTAL, th.P_TOTAL, per_read=True, write_reads=True, reader="device", count_text=fake_count_text(calls))
        assert sorted(fn[len("dev%s" % chunk):] for fn in os.listdir(tmp_path) if fn.startswith("dev%s." % chunk)) == outs
        for tail in outs:
            assert open(prefix + tail, "rb").read() == open(host + tail, "rb").read(), (chunk, tail)
        assert (chunk is None) == (len(calls) <= 2 * len(paths))       # (a FASTA file's last record waits for the file's end)
        assert not [fn for fn in os.listdir(tmp_path) if fn.endswith(".tmp")]


@pytest.mark.parametrize("name,data,message", th.MALFORMED)
def test_malformed_record_has_the_host_readers_words(tmp_path, capsys, monkeypatch, name, data, message):
    from jasper_amd import triobin
    th.write_formats(tmp_path)
    (tmp_path / name).write_bytes(data)
    paths = [str(tmp_path / "a.fq"), str(tmp_path / name)]
    said = []
    for reader, chunk in (("host", None), ("device", None), ("device", 9)):
        if chunk:
            monkeypatch.setenv("JASPER_TRIOBIN_CHUNK", str(chunk))
        before = set(os.listdir(tmp_path))
        with pytest.raises(SystemExit) as e:
            triobin.bin_files(paths, str(tmp_path / "out"), th.ref_counter(), th.M_TOTAL, th.P_TOTAL, per_read=True, write_reads=True, reader=reader,
                              count_text=fake_count_text())
        assert e.value.code == 1
        said.append(capsys.readouterr().err.split("] ", 1)[1])      # (without the time in front)
        assert message in said[-1] and set(os.listdir(tmp_path)) == before
    assert said[0] == said[1] == said[2]


def test_second_pass_notices_a_changed_file(tmp_path, capsys):
    from jasper_amd import triobin
    data = ref.fastq_text(th.READS)
    path = tmp_path / "a.fq"
    shifted = data.replace(b"@", b"@x", 1)[:len(data)]  # the same length, every later record one byte further on
    assert len(shifted) == len(data)
    for changed in (data + ref.fastq_text(th.READS[:1]), data[:-9], shifted):
        path.write_bytes(data)
        inner = fake_count_text()

        def count_text(buf, eof, fmt):
            assert len(buf) == len(data)                # (the first pass has read the whole file)
            (tmp_path / "next").write_bytes(changed)    # (between the two passes: another file under the name, the open one reads on)
            os.replace(tmp_path / "next", path)
            return inner(buf, eof, fmt)

        before = set(os.listdir(tmp_path))
        with pytest.raises(SystemExit) as e:
            triobin.bin_files([str(path)], str(tmp_path / "out"), never, th.M_TOTAL, th.P_TOTAL, write_reads=True, reader="device", count_text=count_text)
        assert e.value.code == 1 and "changed between the two passes" in capsys.readouterr().err
        assert set(os.listdir(tmp_path)) == before


def test_reader_flag_is_checked_before_a_parent_is_opened(capsys, monkeypatch):
    from jasper_amd import triobin
    base = ["-r", "R1.fq", "--mat", "mat.fq", "--pat", "pat.fq"]
    assert triobin.check_reader(triobin.parse_args(base)) == "host"
    assert triobin.check_reader(triobin.parse_args(base + ["--reader", "device"])) == "device"
    assert triobin.check_reader(triobin.parse_args(base + ["--reader", "host"])) == "host"
    with pytest.raises(SystemExit) as e:
        triobin.check_reader(triobin.parse_args(base + ["--reader", "x"]))
    assert e.value.code == 1 and "--reader takes host or device" in capsys.readouterr().err
    for bad in ("0", "-4", "many", str(1 << 30)):
        monkeypatch.setenv("JASPER_TRIOBIN_CHUNK", bad)
        with pytest.raises(SystemExit) as e:
            triobin.check_reader(triobin.parse_args(base + ["--reader", "device"]))
        assert e.value.code == 1 and "JASPER_TRIOBIN_CHUNK" in capsys.readouterr().err
        assert triobin.check_reader(triobin.parse_args(base)) == "host"
    assert "--reader host|device" in triobin.USAGE and "no effect with --reader device" in triobin.USAGE
