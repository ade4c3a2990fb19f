"""The resume variants of both chain kernels of a decode session on the CPU (tests/emu/session_emu.cpp: the lane-loop build of
csrc/decoder_planes.hpp and csrc/decoder_core.hpp), built with -fsanitize=address,undefined as a stand-alone program and run on
the host.  Every chain of every case is split at every plane boundary -- the top planes by the plain variant, the rest resumed
-- under a round-robin and two seeded random wave schedules and on the thread-per-chain route, and every image must equal the
decoder oracle's.  One transform stage and one segment make the four subbands of an image four chains of half its size; where
that image would be too small to encode, a segment count is searched that cuts a chain of the wanted size out of a subband
(config_for): chain widths 1, 2, 63, 64, 65, 130 (a row is one block, a partial block, several blocks) and heights 1, 2, 3, 14,
30 (the ring has 13 rows: 14 and 30 wrap it, and the loader must wait for rows to retire) -- every width of 63 and more with
the heights 3, 14 and 30; the widths and heights 1 and 2 in the combinations an encoder's segment grid gives (it aims at
square segments: no 1 x 30 or 63 x 1 chain comes out of it).  Tiny chains and sparse frames have
packets below 16 bits: resumed, they take the thread route.  CPU only."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import encoder_batch_cases as ebc
from tests import recon_model as rcm
from tests.decoder_batch_cases import oracle_decode

HERE = os.path.dirname(os.path.abspath(__file__))
WIDTHS, HEIGHTS = (1, 2, 63, 64, 65, 130), (1, 2, 3, 14, 30)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("session_emu") / "session_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-DICER_WAVE_EMU",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "emu", "session_emu.cpp")])
    return exe


def case(orc, plane, stages, filt, segments, bits=16):
    h, w = plane.shape
    rc, stream, _ = (orc.compress if bits == 16 else orc.compress_u8)([plane], stages, filt, segments, 4 * w * h + 4096)
    assert rc == 0
    code, ow, oh, planes = oracle_decode(orc, stream, 1, stages, filt, segments, w * h, bits)
    assert (ow, oh) == (w, h)
    return struct.pack("<8Ii", w, h, 1, stages, filt, segments, bits, len(stream), code) + stream + planes[0][: w * h].astype(np.uint16).tobytes()


def config_for(orc, cw, ch):
    """(image w, image h, segments) of a one-stage image one of whose chains is cw x ch; None: no image of the search has one"""
    for W in ([2 * cw] if cw >= 3 else range(6, 14)):
        for H in ([2 * ch] if ch >= 3 else range(6, 14)):
            for segments in range(1, 33):
                for sw, sh in {((W + 1) // 2, (H + 1) // 2), (W // 2, (H + 1) // 2), ((W + 1) // 2, H // 2), (W // 2, H // 2)}:
                    rects = rcm.rects_of(orc, sw, sh, segments)
                    if rects and any((r[2], r[3]) == (cw, ch) for r in rects):
                        return W, H, segments
    return None                     # (the segment grid aims at square segments: no 1 x 30 chain comes out of an encoder)


def run(program, tmp_path, cases):
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(cases))
    r = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def test_every_shape_split_at_every_plane(program, tmp_path, oracle):
    cases, seen = [], set()
    for i, cw in enumerate(WIDTHS):
        for j, ch in enumerate(HEIGHTS):
            kind = ("noise8", "sparse", "smooth")[(i + j) % 3]
            cfg = config_for(oracle, cw, ch)
            if cfg is None:
                continue
            W, H, segments = cfg
            seen.add((cw, ch))
            cases.append(case(oracle, ebc.plane16(kind, W, H, 10 * i + j), 1, (0, 2)[(i + j) % 2], segments))
    # every width and every height, and every width of 63 and more with the heights 3, 14 and 30 (the ring wraps at 14 and 30)
    assert {c for c, _ in seen} == set(WIDTHS) and {r for _, r in seen} == set(HEIGHTS), sorted(seen)
    assert {(c, r) for c in WIDTHS[2:] for r in HEIGHTS[2:]} <= seen, sorted(seen)
    stats = run(program, tmp_path, cases)
    assert stats["cases"] == len(cases) and stats["runs"] == stats["cases"] * 10 * 4
    assert stats["loader_chains"] > 0 and stats["thread_resumes"] > 0, stats
    assert stats["short_packet_resumes"] > 0, "no resumed chain with a packet below 16 bits took the thread route"
    assert stats["loader_waits"] > 0, "no loader ever waited for a ring slot to be recycled"


def test_odd_sizes_segments_levels_and_8_bit(program, tmp_path, oracle):
    cases = [case(oracle, ebc.plane16("noise8", 129, 61, 1), 1, 0, 1),          # chains of 65 and 64 by 31 and 30
             case(oracle, ebc.plane16("wide", 200, 72, 2), 3, 0, 4),           # three levels, four segments per subband
             case(oracle, ebc.plane16("smooth", 140, 50, 3), 2, 2, 3),
             case(oracle, ebc.plane8("noise6", 132, 60, 4), 1, 0, 1, bits=8),
             case(oracle, ebc.plane8("smooth6", 96, 80, 5), 3, 0, 3, bits=8)]
    stats = run(program, tmp_path, cases)
    assert stats["cases"] == len(cases) and stats["loader_chains"] > 0 and stats["loader_waits"] > 0, stats
