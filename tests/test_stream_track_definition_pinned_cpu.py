"""The numpy definition of the stream tracker (dagr_amd/streaming.py: TrackDefinition), pinned: a SHA-256 over the raw
bytes of everything a step leaves, after every step of the seeded walks, against the digests recorded from the definition
as it stood when the plain and the motion step were two separate functions.  Every operation is elementwise fp32 / int64
numpy without a transcendental, so the bytes do not depend on the machine."""
import hashlib

import numpy as np
import pytest

from tests import stream_motion_cases as mc
from tests import stream_track_cases as tc


def _feed(h, *arrays):
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())


def plain_digest(case):
    """ids, hits, untracked, then the slot arrays (id, t_last, box, label, hits, next_id), step by step."""
    h = hashlib.sha256()
    for ids, hits, untracked, slots in tc.run_definition(case)[0]:
        _feed(h, ids, hits, untracked, *slots)
    return h.hexdigest()


def motion_digest(case):
    """ids, hits, untracked, the slot arrays (id, t_last, box, vel, label, hits, next_id), track_box, track_vel, n_coast
    and, lane by lane, the first n_coast[b] entries of coast id, box, label and age, step by step."""
    h = hashlib.sha256()
    for s in mc.run_definition(case)[0]:
        _feed(h, s["ids"], s["hits"], s["untracked"], *s["slots"], s["box"], s["vel"], s["n_coast"])
        for b, n in enumerate(s["n_coast"]):
            _feed(h, *[a[b, :n] for a in s["coast"]])
    return h.hexdigest()


PLAIN = {8: "554ffe0682393ef62296841a5f83a70520bb1fa83941f5ad9f1f9aaa56b5eee0",
         64: "e380ec7e6357bf39d8b599b5d02dd005e3fd89af9053a27366085856b4f6b3a4"}
MOTION = {("walk", 8): "96429198b4428270d3b70754fd0233690a11bdee31a2450c7a4cbc49b1a8bd83",
          ("walk", 64): "4c40747efc8b10c2c93e37eba71348de6874df8e65b5e4f1e635bb32aedfec0c",
          ("walk", 130): "824f5de5ebc6297e467020a1b58f77a136b263a86f27f89c6ff70e86000703ab",
          ("shared", 8): "db1e24eec1a5f19f54ba67f88016bd5e424f4d92ad0db4feb79e586a5e049ac5",
          ("shared", 64): "65d657d78b5524a5760c953f35cba55b53906429bc468c939c932b17802a7e1c"}


@pytest.mark.parametrize("max_tracks", sorted(PLAIN))
def test_the_plain_definition_gives_the_recorded_bytes(max_tracks):
    assert plain_digest(tc.random_walk(max_tracks)) == PLAIN[max_tracks]


@pytest.mark.parametrize("kind,max_tracks", sorted(MOTION))
def test_the_motion_definition_gives_the_recorded_bytes(kind, max_tracks):
    case = mc.random_walk(max_tracks) if kind == "walk" else mc.shared_instant(max_tracks)
    assert motion_digest(case) == MOTION[(kind, max_tracks)]
