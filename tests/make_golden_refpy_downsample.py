#!/usr/bin/env python
"""Golden outputs of the reference's OWN ``scripts/downsample_events.py`` at cell areas that are no power of two, executed on
CPU (build container only: it loads /root/reference/scripts/downsample_events.py by path, numba stubbed with identity
decorators as in tests/make_golden_refpy_data.py).  Writes tests/golden/ref_py_downsample_factors.npz; the inputs are
tests/downsample_factor_cases.py's and are not stored.  Per case ``(fx, fy)``:

  * ``{fx}x{fy}_sha256``            sha256 of the concatenated input arrays
  * ``{fx}x{fy}_mask0``, ``_mask1`` the reference's kept mask of each chunk, ``np.packbits``
  * ``{fx}x{fy}_map0``, ``_map1``   the change map after each chunk, fp32 [6, 8]

A fixture that could not tell the reference's increment (the float64 quotient ``p * 1.0 / (fx * fy)``) from one rounded to
fp32 before it is used would pin nothing, so the fp32 increment is restated below and has to DISAGREE with the reference on
every case but the control: in the kept set at areas 3, 6 and 15, at least in the final map at areas 9, 12 and 25.  The
generator refuses to write otherwise."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import downsample_factor_cases as fc  # noqa: E402

REFERENCE_SCRIPT = "/root/reference/scripts/downsample_events.py"


def fp32_increment_loop(chunks, fx, fy):
    """The arithmetic the fixture has to tell from the reference's: the increment rounded to fp32 first, then a float64
    multiply-add rounded into the fp32 cell.  Per chunk ``(mask, map)``."""
    inc = float(np.float32(1.0 / (fx * fy)))
    cm = np.zeros((fc.CH, fc.CW), np.float32)
    out = []
    for ev in chunks:
        cx, cy, p = (ev["x"] // fx).tolist(), (ev["y"] // fy).tolist(), ev["p"].tolist()
        mask = np.zeros(len(p), bool)
        for i in range(len(p)):
            state = np.float32(float(cm[cy[i], cx[i]]) + p[i] * inc)
            if abs(state) >= 1:
                mask[i] = True
                state = np.float32(state - np.float32(p[i]))
            cm[cy[i], cx[i]] = state
        out.append((mask, cm.copy()))
    return out


def load_reference():
    from tests.make_golden_refpy_data import install_stubs
    install_stubs()
    spec = importlib.util.spec_from_file_location("ref_downsample", REFERENCE_SCRIPT)
    rds = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rds)
    return rds


def main():
    rds = load_reference()
    out = {}
    for fx, fy in fc.CASES:
        area, tag = fx * fy, f"{fx}x{fy}"
        chunks = fc.chunks(fx, fy)
        out[f"{tag}_sha256"] = fc.digest(fx, fy)
        cm, masks, maps = None, [], []
        for c, ev in enumerate(chunks):
            ids = np.arange(len(ev["t"]))
            res, cm = rds.downsample_events(dict(ev, i=ids), fc.CH * fy, fc.CW * fx, fc.CH, fc.CW, change_map=cm)
            assert cm.dtype == np.float32 and cm.shape == (fc.CH, fc.CW)
            mask = np.zeros(len(ids), bool)
            mask[res["i"]] = True
            assert np.array_equal(res["x"], ev["x"][mask] // fx) and np.array_equal(res["y"], ev["y"][mask] // fy)
            masks.append(mask)
            maps.append(cm.copy())
            out[f"{tag}_mask{c}"], out[f"{tag}_map{c}"] = np.packbits(mask), cm.copy()
        old = fp32_increment_loop(chunks, fx, fy)
        kept_differs = any(not np.array_equal(m, o[0]) for m, o in zip(masks, old))
        n_kept = sum(int((m != o[0]).sum()) for m, o in zip(masks, old))
        map_cells = int((maps[-1] != old[-1][1]).sum())
        print(f"{tag}: area {area:2d}, kept {[int(m.sum()) for m in masks]} of {[len(m) for m in masks]}; the fp32 increment "
              f"differs on {n_kept} kept flags and in {map_cells} of {fc.CW * fc.CH} final cells")
        if (fx, fy) == fc.CONTROL:
            assert not kept_differs and map_cells == 0, f"{tag}: the control tells the two arithmetics apart"
        elif area in fc.KEPT_SET_DIFFERS:
            assert kept_differs, f"{tag}: the kept set does not tell the fp32 increment from the reference's"
        else:
            assert area in fc.FINAL_MAP_DIFFERS
            assert map_cells > 0, f"{tag}: the final map does not tell the fp32 increment from the reference's"
    path = os.path.join(os.environ.get("GOLDEN_OUT", os.path.dirname(fc.FIXTURE)), os.path.basename(fc.FIXTURE))
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
