"""The resumable lane-per-plane chain decoder of a decode session on the CPU (tests/emu/session_wave_emu.cpp: the lane-loop build
of csrc/decoder_wave.hpp decode_chain_wave_resume), built with -fsanitize=address,undefined as a stand-alone program and run on
the host.  Every chain of every case is split at every plane boundary -- the top planes by decode_chain_wave, the rest resumed in
place on the same plane, no plane held included -- and every image must equal the decoder oracle's; per resumed chain the program
also holds lowest_ok and the plane against decode_chain_resume and checks that the held bits are intact.  The cases are those of
tests/test_session_emu.py: chain widths 1, 2, 63, 64, 65, 130 and heights 1, 2, 3, 14, 30 -- the ring of a 16-bit chain has 13
rows, so the heights 14 and 30 recycle slots, which then take their rows from the state plane -- and its odd sizes, levels,
segments and 8-bit frames.  The damaged cases have a packet whose entropy decode fails (its header's length cut to one bit, or to
4 or 5 bits -- late enough for the planes below it to have started: they are rolled back --, both CRCs recomputed).  CPU only."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import encoder_batch_cases as ebc
from tests import reduced_model as red
from tests import session_cases as sc
from tests import test_session_emu as tse
from tests.decoder_batch_cases import oracle_decode

HERE = os.path.dirname(os.path.abspath(__file__))
NO_PACKET = 0xFFFFFFFF


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("session_wave_emu") / "session_wave_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-DICER_WAVE_EMU",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "emu", "session_wave_emu.cpp")])
    return exe


def record(orc, stream, w, h, stages, filt, segments, bits=16, fail_off=NO_PACKET):
    code, ow, oh, planes = oracle_decode(orc, stream, 1, stages, filt, segments, w * h, bits)
    assert (ow, oh) == (w, h)
    return struct.pack("<8IiI", w, h, 1, stages, filt, segments, bits, len(stream), code, fail_off) + stream + planes[0][: w * h].astype(np.uint16).tobytes()


def case(orc, plane, stages, filt, segments, bits=16):
    h, w = plane.shape
    rc, stream, _ = (orc.compress if bits == 16 else orc.compress_u8)([plane], stages, filt, segments, 4 * w * h + 4096)
    assert rc == 0
    return record(orc, stream, w, h, stages, filt, segments, bits)


def run(program, tmp_path, cases):
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(cases))
    r = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def test_every_shape_split_at_every_plane(program, tmp_path, oracle):
    cases, seen = [], set()
    for i, cw in enumerate(tse.WIDTHS):
        for j, ch in enumerate(tse.HEIGHTS):
            kind = ("noise8", "sparse", "smooth")[(i + j) % 3]
            cfg = tse.config_for(oracle, cw, ch)
            if cfg is None:
                continue
            W, H, segments = cfg
            seen.add((cw, ch))
            cases.append(case(oracle, ebc.plane16(kind, W, H, 10 * i + j), 1, (0, 2)[(i + j) % 2], segments))
    assert {c for c, _ in seen} == set(tse.WIDTHS) and {r for _, r in seen} == set(tse.HEIGHTS), sorted(seen)
    assert {(c, r) for c in tse.WIDTHS[2:] for r in tse.HEIGHTS[2:]} <= seen, sorted(seen)
    stats = run(program, tmp_path, cases)
    assert stats["cases"] == len(cases) and stats["runs"] == stats["cases"] * 10
    assert stats["resumes"] > 0 and stats["fresh_runs"] > 0, stats
    # (every call with no plane held was repeated by decode_chain_wave: the same words, the same schedule counts)
    assert stats["plain_checked"] == stats["fresh_runs"], stats
    assert stats["reloaded_rows"] > 0, "no recycled ring slot ever took a row of the state plane"
    assert stats["rollbacks"] == 0 and stats["stops"] == 0, stats


def test_odd_sizes_segments_levels_and_8_bit(program, tmp_path, oracle):
    cases = [case(oracle, ebc.plane16("noise8", 129, 61, 1), 1, 0, 1),          # chains of 65 and 64 by 31 and 30
             case(oracle, ebc.plane16("wide", 200, 72, 2), 3, 0, 4),           # three levels, four segments per subband
             case(oracle, ebc.plane16("smooth", 140, 50, 3), 2, 2, 3),
             case(oracle, ebc.plane8("noise6", 132, 60, 4), 1, 0, 1, bits=8),   # (kPlanes8: a ring of 11 rows under chains of 30)
             case(oracle, ebc.plane8("smooth6", 96, 80, 5), 3, 0, 3, bits=8)]
    stats = run(program, tmp_path, cases)
    assert stats["cases"] == len(cases) and stats["runs"] == 3 * 10 + 2 * 8, stats
    assert stats["resumes"] > 0 and stats["reloaded_rows"] > 0 and stats["stops"] == 0, stats


def failing_streams(orc, stream, w, h, stages, filt, segments, bits, most, wanted=lambda level, lsb: True):
    """streams with one packet cut to `bits` bits (tests/session_cases.py shorten_packet) such that the oracle shows the chain stopping
    there -- the image is the same without the chain's lower planes, and is not the clean one -- and planes of the chain above and
    below it: [(stream, offset of the packet)], of the packets that wanted(level, bit plane) picks"""
    dec = lambda s: oracle_decode(orc, s, 1, stages, filt, segments, w * h, 16)
    same = lambda a, b: a[:3] == b[:3] and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    clean = dec(stream)
    found = []
    for which, (off, n) in enumerate(red.walk(stream)):
        crafted, _ = sc.shorten_packet(stream, which, bits)             # (the packets in front of it stay where they are)
        key, lsb = crafted[off + 4: off + 7], crafted[off + 7] & 15
        chain = [(o, m) for o, m in red.walk(crafted) if crafted[o + 4: o + 7] == key]
        below = [(o, m) for o, m in chain if (crafted[o + 7] & 15) < lsb]
        if not wanted(key[0], lsb) or not below or not any((crafted[o + 7] & 15) > lsb for o, m in chain):
            continue
        without = b"".join(crafted[o: o + m] for o, m in red.walk(crafted) if (o, m) not in below)
        full = dec(crafted)
        if same(full, dec(without)) and not same(full, clean):
            found.append((crafted, off))
            if len(found) == most:
                break
    return found


def test_a_failing_plane_below_held_planes_is_reported_and_rolled_back(program, tmp_path, oracle):
    """A packet cut to one bit fails at the first code word of bins 1 to 7, two or three samples into its plane: the plane below it
    has not started by then (it wants the plane above w + 2 samples ahead), so there is nothing to take back -- the program checks the
    stop report, the held bits and the image.  For the roll-back a packet of a middle plane is cut to 4 or 5 bits, as
    tests/test_emu_decoder.py does it: the decoder then refuses the first code word of that length, which comes up some rows in."""
    w, h, stages, filt, segments = 96, 80, 1, 0, 2
    rc, stream, _ = oracle.compress([ebc.plane16("noise8", w, h, 7)], stages, filt, segments, 4 * w * h + 4096)
    assert rc == 0
    one_bit = failing_streams(oracle, stream, w, h, stages, filt, segments, 1, 2)
    assert one_bit, "no packet of the stream cut to one bit makes the oracle stop a chain"
    stats = run(program, tmp_path, [record(oracle, s, w, h, stages, filt, segments, fail_off=off) for s, off in one_bit])
    # (the program has checked, per chain: lowest_ok = the plane above the failing packet, the held bits intact, the oracle's image)
    assert stats["cases"] == len(one_bit) and stats["resumes"] > 0 and stats["reloaded_rows"] > 0 and stats["stops_below_held"] > 0, stats
    # the small chains of the deepest level: the planes lie a few samples apart
    w, h, stages, filt, segments = 200, 72, 3, 0, 4
    rc, stream, _ = oracle.compress([ebc.plane16("wide", w, h, 7)], stages, filt, segments, 4 * w * h + 4096)
    assert rc == 0
    later = [x for bits in (4, 5) for x in failing_streams(oracle, stream, w, h, stages, filt, segments, bits, 3, lambda level, lsb: level == 3 and lsb <= 5)]
    assert later, "no packet of the stream cut to 4 or 5 bits makes the oracle stop a chain"
    stats = run(program, tmp_path, [record(oracle, s, w, h, stages, filt, segments, fail_off=off) for s, off in later])
    assert stats["cases"] == len(later) and stats["resumes"] > 0 and stats["stops_below_held"] > 0, stats
    assert stats["rollbacks"] > 0 and stats["rollbacks_below_held"] > 0, stats
