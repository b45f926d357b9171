"""GPU: the device inflater (jasper_amd/csrc/inflate_gpu.hip) on streams that zlib's deflate never writes, and on streams that are
wrong in one chosen way.  The streams and what zlib makes of each are the CASES of tests/test_deflate_writer.py (pinned there
without a GPU); here every one goes through jasper_inflate_file_device with the smallest decoder chunk, 4096 compressed bytes, so a
stream of 100 KB is tens of decoders.  Text must be zlib's byte for byte, verdicts must be zlib's, and for a DEVICE case the host's
share must be zero: an arena that overflows hands the work to zlib on the host, which would hide a wrong device decoder.
"""
import pytest

from test_deflate_writer import CASES, CHUNK, DEVICE, MEMBERS, VALID, WRONG
from test_gpu_inflate import dev_inflate, host_inflate

pytestmark = pytest.mark.gpu


def run(L, tmp_path, name):
    blob, text = CASES[name]
    p, out = tmp_path / "in.gz", tmp_path / "out"
    p.write_bytes(blob)
    rc, n, st = dev_inflate(L, p, out, chunk=CHUNK)
    print(name, "rc", rc, "n", n, st)
    return rc, n, st, out


@pytest.mark.parametrize("name", VALID)
def test_valid_stream(hip, tmp_path, name):
    text = CASES[name][1]
    rc, n, st, out = run(hip, tmp_path, name)
    assert rc == 0, st
    assert n == len(text) and out.read_bytes() == text
    assert st["members"] == MEMBERS[name] and st["device_bytes"] + st["host_bytes"] == len(text), st
    assert st["accepted"] <= st["decoders"], st
    if name in DEVICE:
        assert st["host_bytes"] == 0 and st["device_bytes"] == len(text), st


def test_chunk_starts_were_taken(hip, tmp_path):
    """what the counters must say where a case is about chunk starts"""
    # several far_matches blocks were chunk starts: the markers 256 + 0 and 256 + 32767 went through the window and resolve kernels
    assert run(hip, tmp_path, "far_matches")[2]["accepted"] >= 10
    # the block that looks 50 bytes back was a chunk start (the same block looks 200 back in too_far_back_at_chunk_start)
    st = run(hip, tmp_path, "chunk_start_twin_distance_50")[2]
    assert st["accepted"] >= 2 and st["decoders"] == 2, st
    rc, _, st, _ = run(hip, tmp_path, "too_far_back_at_chunk_start")
    assert rc != 0 and st["decoders"] == 2, st
    # the inner stream's headers were candidate starts, decoded, and never on the chain
    for name in ("nested_gzip", "nested_gzip_4k_members"):
        st = run(hip, tmp_path, name)[2]
        assert st["decoders"] > st["accepted"], st


@pytest.mark.parametrize("name", WRONG)
def test_wrong_stream_is_refused(hip, tmp_path, name):
    """every wrong block is followed by a good last block and a real trailer, so running off the data refuses nothing; for the
    LENIENT cases of the table the trailer is that of the text a decoder without the check would give, so there only the check
    itself can say no.  The others (a code that cannot be assigned, a symbol that stands for nothing) have no such text."""
    rc, n, st, out = run(hip, tmp_path, name)
    rc_h, _, _ = host_inflate(hip, tmp_path / "in.gz")
    assert rc != 0 and rc_h != 0, (rc, rc_h, st)
