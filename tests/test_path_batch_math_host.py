"""The integer geometry of batched path IK (ikflow_amd/csrc/path_batch_math.h: where a path begins in the candidate layout of P * T waypoints, the
back-pointer blocks, the mask words, the role of a sweep wave) compiled for the HOST with g++ and held against plain Python - the kernels' own
source, checked without a GPU.  The GPU tests check the same code where it ships (tests/test_path_batch.py).  Test infrastructure: nothing in
ikflow_amd/ loads it."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (3, 1, 5), (3, 3, 5), (2, 2, 17), (5, 3, 64), (2, 5, 129), (4, 65, 33), (2, 66, 256), (300, 4, 6), (7, 1, 255)]


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("path_batch_math") / "libpath_batch_math_host.so"
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas",
           os.path.join(ROOT, "tests", "path_batch_math_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(out))
    LL, I = C.c_longlong, C.c_int
    sigs = {"pbm_waypoints": [LL, LL], "pbm_offset": [LL, LL], "pbm_row": [LL, LL, LL, LL, I], "pbm_bp_stride": [LL, I], "pbm_bp_offset": [LL, LL, I],
            "pbm_bp_bytes": [LL, LL, I], "pbm_single_bp_bytes": [LL, I], "pbm_mask_offset": [LL, LL, I], "pbm_pred_row": [LL, LL, LL, I],
            "pbm_word_index": [LL, I, I, I], "pbm_mask_words": [LL, I], "pbm_chunk_words": [I, I]}
    for name, args in sigs.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = LL
    lib.pbm_wave_role.argtypes = [LL, LL, I, C.POINTER(LL)]
    lib.pbm_wave_role.restype = None
    return lib


@pytest.mark.parametrize("P,T,k", SHAPES)
def test_offsets_and_strides(host_lib, P, T, k):
    """Row r * (P * T) + p * T + t; the rows of path p gathered in (r, t) order are its own k x T tile-major lattice; the rows of all paths
    partition 0 .. k * P * T - 1; the predecessor row of a wave at g is candidate j of waypoint g - 1."""
    lib = host_lib
    assert lib.pbm_waypoints(P, T) == P * T
    seen = set()
    for p in range(P):
        assert lib.pbm_offset(p, T) == p * T
        for r in (0, k // 2, k - 1):
            for t in (0, T // 2, T - 1):
                row = lib.pbm_row(P, T, p, t, r)
                assert row == r * (P * T) + p * T + t
                if t > 0:
                    for j in (0, k - 1):
                        assert lib.pbm_pred_row(P, T, p * T + t, j) == lib.pbm_row(P, T, p, t - 1, j)
    if k * P * T <= 20000:
        for p, r, t in itertools.product(range(P), range(k), range(T)):
            seen.add(lib.pbm_row(P, T, p, t, r))
        assert seen == set(range(k * P * T))


@pytest.mark.parametrize("P,T,k", SHAPES + [(3, 3, 5), (5, 7, 3), (4, 1, 1)])
def test_back_pointer_blocks_are_word_aligned_and_disjoint(host_lib, P, T, k):
    """A path's block starts on a 4-byte boundary (T * k = 15 at (3, 3, 5) would not), is the single path's path_bp_bytes, holds the T * k bytes
    the search writes and every whole word the walk back reads - chunk by chunk, (n k + 3) / 4 words from byte tc * k - and ends where the next
    block begins."""
    lib = host_lib
    stride = lib.pbm_bp_stride(T, k)
    assert stride == lib.pbm_single_bp_bytes(T, k) and stride % 4 == 0 and stride >= T * k
    assert lib.pbm_bp_bytes(P, T, k) == P * stride
    chunk = lib.pbm_bt_chunk()
    for p in range(P):
        off = lib.pbm_bp_offset(p, T, k)
        assert off == p * stride and off % 4 == 0
        assert off + stride <= lib.pbm_bp_bytes(P, T, k)
        for tc in range(0, T, chunk):
            n = min(chunk, T - tc)
            assert (tc * k) % 4 == 0                                   # (a chunk starts on a word of its block)
            last_byte_read = tc * k + 4 * lib.pbm_chunk_words(n, k)
            assert last_byte_read <= stride, (p, tc, last_byte_read, stride)
    if T * k % 4:
        assert (T * k) % 4 != 0 and lib.pbm_bp_offset(1, T, k) != T * k   # the unpadded stride would leave path 1 misaligned


@pytest.mark.parametrize("P,T,k", SHAPES)
def test_sweep_wave_role_inverts_the_word_index_over_a_batch(host_lib, P, T, k):
    """Wave w of the sweep's lattice source over P * T waypoints writes word w of the mask; its role is (p, t, r, word) with
    sweep_word_index(p * T + t, r, word, k) == w; the words of path p begin at path_batch_mask_offset(p) and are those of a single lattice from
    there on; every wave of the launch has exactly one role."""
    lib = host_lib
    words = (k + 63) // 64
    total = lib.pbm_mask_words(P * T, k)
    assert total == P * T * k * words
    out = (C.c_longlong * 4)()
    waves = range(total) if total <= 40000 else list(range(0, total, 97)) + [total - 1]
    roles = set()
    for w in waves:
        lib.pbm_wave_role(w, T, k, out)
        p, t, r, word = (int(x) for x in out)
        assert 0 <= p < P and 0 <= t < T and 0 <= r < k and 0 <= word < words
        assert lib.pbm_word_index(p * T + t, r, word, k) == w
        assert lib.pbm_mask_offset(p, T, k) + lib.pbm_word_index(t, r, word, k) == w
        roles.add((p, t, r, word))
    assert len(roles) == len(waves)
    for p in range(P):   # the first wave of a path is a start edge (t == 0), the one in front of it the LAST waypoint of the path before
        lib.pbm_wave_role(lib.pbm_mask_offset(p, T, k), T, k, out)
        assert (int(out[0]), int(out[1]), int(out[2]), int(out[3])) == (p, 0, 0, 0)
        if p > 0:
            lib.pbm_wave_role(lib.pbm_mask_offset(p, T, k) - 1, T, k, out)
            assert (int(out[0]), int(out[1]), int(out[2]), int(out[3])) == (p - 1, T - 1, k - 1, words - 1)
