"""Writes tests/golden/gpuhc_p2c_N100_seed0.npz from the P2C restatement
(tests/p2c_ref): config 2 (dataset 000, srand(0), 100 samples) with the
reference's P2C tables (tests/golden/p2c), the map derived from them and the
generator's coefficient blocks.  Flags, step counts and track hashes, like
gpuhc_ph_N100_seed0.npz.  Run from the repository root after build():
    python tests/golden/make_golden_p2c.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import checks  # noqa: E402
import p2c_common as pc  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    tr, conv, inf, st = pc.ref_track(100)
    counts = np.array(O.count_solutions(tr, conv, inf), np.int64)
    np.savez_compressed(os.path.join(HERE, "gpuhc_p2c_N100_seed0.npz"), conv=conv, inf=inf,
                        steps=st["steps"].astype(np.int16), corrections=st["corrections"].astype(np.int16),
                        hash=checks.track_hash(tr), counts=counts)
    print(f"P2C N=100 seed 0: converged / real / inf = {counts.tolist()}, mean steps per path {st['steps'].mean():.3f}")


if __name__ == "__main__":
    main()
