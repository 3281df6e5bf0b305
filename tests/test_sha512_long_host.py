"""The host side of the long SHA-512 / SHA-384 path
(firedancer_amd/csrc/fd_sha512_gpu_pack.h): the padded byte stream a
message is moved to the device as, and the geometry of the pinned blob it
moves through.  tests/sha_long_pack_harness.cpp is a stand-alone program
with its own main, built with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process: nothing is preloaded
and nothing is loaded into Python.  Each message is a heap block of exactly
its size and each piece a heap block of exactly the piece, so a read or a
write one byte outside either is caught."""
import os
import struct
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "sha_long_pack_harness.cpp")
INC = os.path.join(ROOT, "firedancer_amd", "csrc")
SIZES = ((0, 400), (2049, 2176))      # every size to 400; all 128 tail residues past a 2,048-byte blob


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("sha_long") / "sha_long_pack"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, SRC, "-o", str(out)], check=True, capture_output=True)
    return str(out)


def run(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err
    assert "runtime error" not in err and "AddressSanitizer" not in err, err
    return r.stdout


def message(sz):
    return bytes((i * 131 + 7) & 255 for i in range(sz))


def padded(msg, sz=None):
    """M || 0x80 || 0.. || bitlen128, built here (FIPS 180-4 5.1.2)"""
    sz = len(msg) if sz is None else sz
    zeros = (-(sz + 17)) % 128
    return msg + b"\x80" + b"\0" * zeros + (sz * 8).to_bytes(16, "big")


def streams(raw):
    out, o = [], 0
    while o < len(raw):
        (n,) = struct.unpack_from("<Q", raw, o)
        out.append(raw[o + 8:o + 8 + n])
        o += 8 + n
    assert o == len(raw)
    return out


CUTS = [("128",)] + [("geo", blob, 64, m) for blob in (2048, 3000) for m in (1, 0)]     # m 0: a full group, m = G


@pytest.mark.parametrize("cut", CUTS, ids=lambda c: "-".join(str(x) for x in c))
def test_padded_stream_in_pieces(exe, cut):
    for lo, hi in SIZES:
        got = streams(run(exe, "stream", lo, hi, *cut))
        assert len(got) == hi - lo + 1
        for sz, g in zip(range(lo, hi + 1), got):
            assert g == padded(message(sz)), (cut, sz)


@pytest.mark.parametrize("sz", [1 << 32, (1 << 32) + 128, 1 << 61, (1 << 61) + (1 << 32)])
def test_sizes_nobody_can_allocate(exe, sz):
    """the last block of a stream whose length is a multiple of 128 holds no
    message byte: packed from a NULL message it is the padding bit, zeros and
    the exact 128-bit count, whose high word is sz >> 61"""
    got = run(exe, "tail", sz)
    assert got == b"\x80" + b"\0" * 111 + (sz * 8).to_bytes(16, "big")
    assert got == padded(b"", sz)[-128:]
    if sz >= 1 << 61:
        assert int.from_bytes(got[112:120], "big") == sz >> 61 != 0
    assert int.from_bytes(got[112:128], "big") >> 32 != 0          # past a 32-bit bit count in every case


def test_geometry_every_blob(exe):
    out = run(exe, "geometry", 100, 20000).decode()
    assert out.strip().endswith("geometry ok"), out
    assert int(out.split()[0]) > 100000, out
