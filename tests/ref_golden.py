"""Digests of what the reference's own kernels (oracle/_ref) return in the GPU tests that compare against them bit for bit.

Where oracle/_ref is built, ``reference`` runs the reference kernels and digests their output; elsewhere it returns the
digest stored in tests/golden/ref_kernels_sha256.json, so the comparison runs on every checkout.  To regenerate the file,
run those tests on a GPU with oracle/_ref built and ``DAGR_REF_GOLDEN_OUT=<path of the new file>``."""
import hashlib
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kernels_sha256.json")


def digest(a):
    """sha256 over dtype, shape and bytes of a tensor or array."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


def reference(key, available, run_reference):
    """Digest of the reference kernels' output for ``key``: ``run_reference()`` when ``available``, else the stored one."""
    if not available:
        with open(GOLDEN) as f:
            stored = json.load(f)
        assert key in stored, f"{key}: no stored digest in {GOLDEN}"
        return stored[key]
    d = digest(run_reference())
    out = os.environ.get("DAGR_REF_GOLDEN_OUT")
    if out:
        rec = {}
        if os.path.exists(out):
            with open(out) as f:
                rec = json.load(f)
        rec[key] = d
        with open(out, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    return d
