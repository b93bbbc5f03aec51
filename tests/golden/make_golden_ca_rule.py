"""
Writes tests/golden/ca_rule_cases.npz: what the REFERENCE's compiled speedups.advance_board and life_occupancy make of
the constructed boards of tests/ca_rule_cases.py, for tests/test_ca_rule_host.py (the restatement tests/ca_ref.py must
reproduce every array) and tests/test_ca_rule_gpu.py.

Run once on a CPU with the reference extension built (``make -C oracle ref``, then
``python tests/golden/make_golden_ca_rule.py``) and commit the output.  Every board is one call of its own on a numpy
PCG64 set to the board's words; the generator's words after the call are recorded.

    cases                 names: "<kind>-<H>x<W>" -- every tile board at 25x25; the seam boards at 25x25, 64x64 and 9x11;
                          soup boards at five shapes
    <case>_in, _p, _w0    the boards uint16 [B, H, W], their spawn_prob float32 [B], generator words uint64 [B, 4] before
    <case>_adv<n>, _adv<n>_w     advance_board(board, p, n), n = 1 and 3, and the words after
    <case>_occ<n>, _occ<n>_w     life_occupancy(board, p, n), n = 1, 2 and 7 (uint8: no count exceeds n), words after
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle                                   # noqa: E402
from tests import ca_rule_cases as crc          # noqa: E402

ADVANCE_N, OCCUPANCY_N = (1, 3), (1, 2, 7)


def fixture_cases():
    return ([("tile",) + crc.FIXTURE_TILE_SHAPE] + [("seam",) + s for s in crc.FIXTURE_SEAM_SHAPES]
            + [("soup",) + s for s in crc.FIXTURE_SOUP_SHAPES])


def main():
    oracle.build()
    sp = oracle.load_ref()
    assert sp is not None, "run `make -C oracle ref` first"
    bg = np.random.PCG64(0)
    sp.set_bit_generator(bg)
    out = {"cases": np.array([crc.case_id(c) for c in fixture_cases()])}
    for case in fixture_cases():
        kind, H, W = case
        name = crc.case_id(case)
        b = crc.BATCHES[kind](H, W)
        B = len(b.boards)
        out[name + "_in"], out[name + "_p"], out[name + "_w0"] = b.boards, b.p, b.words

        def call(fn, n, dtype, shape):
            res, words = np.zeros((B,) + shape, dtype), np.zeros((B, 4), np.uint64)
            for k in range(B):
                oracle.pcg64_set_state_words(bg, b.words[k])
                got = fn(np.array(b.boards[k]), float(b.p[k]), n)
                assert got.max() <= np.iinfo(dtype).max
                res[k], words[k] = got, oracle.pcg64_state_words(bg)
            return res, words

        for n in ADVANCE_N:
            out["%s_adv%d" % (name, n)], out["%s_adv%d_w" % (name, n)] = call(sp.advance_board, n, np.uint16, (H, W))
        for n in OCCUPANCY_N:
            out["%s_occ%d" % (name, n)], out["%s_occ%d_w" % (name, n)] = call(sp.life_occupancy, n, np.uint8, (H, W, 8))
        print(name, B, "boards")
    path = os.path.join(HERE, "ca_rule_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
