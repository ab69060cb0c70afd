#!/usr/bin/env python
"""Record which kernel engine.Lowering.conv3_route gives a stride-1 3x3 convolution over a grid of environment switches, batches
and layer shapes (CPU only, no library): tests/golden/conv3_routes.json, which tests/test_host_cpu.py recomputes and compares.
Run it on the commit whose decisions are to be kept, BEFORE a change that is meant to leave them alone.

The file holds the grid axes, `tiles` (the TILE_* values that occur) and, per combination of switches and batch
("SSDE_WINOGRAD/SSDE_CONV_KSPLIT/SSDE_WINO4_TWO/SSDE_NUM_CUS/batch"), one string with a digit per (hw, c_out, c_in, aux) point,
last axis fastest: the index into `tiles` of the chosen route's tile.
usage: record_conv3_routes.py [out.json]"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AXES = dict(SSDE_WINOGRAD=["0", "1", "2", "3", "4"], SSDE_CONV_KSPLIT=["1", "0"], SSDE_WINO4_TWO=["2", "0"],
            SSDE_NUM_CUS=["256", "128"], batch=[1, 15, 16, 128, 256], hw=[4, 6, 8, 12, 16, 32], c_out=[4, 32, 64, 256],
            c_in=[4, 12, 16, 128, 256, 512], aux=[False, True])
SWITCHES = ("SSDE_WINOGRAD", "SSDE_CONV_KSPLIT", "SSDE_WINO4_TWO", "SSDE_NUM_CUS")


def record(axes=AXES):
    """{combination key: [tile per (hw, c_out, c_in, aux) point]}; sets the switches in os.environ and restores them."""
    import torch
    from score_sde_pytorch_amd import engine as E
    saved = {k: os.environ.get(k) for k in SWITCHES}
    out = {}
    try:
        for combo in itertools.product(*[axes[k] for k in SWITCHES]):
            os.environ.update(dict(zip(SWITCHES, combo)))
            for n in axes["batch"]:
                low = E.Lowering(E.ProgramBuilder(torch.device("cpu")), None, n)
                out["/".join(combo + (str(n),))] = [
                    low.conv3_route(hw, hw, c_out, c_in, aux=aux).tile
                    for hw, c_out, c_in, aux in itertools.product(axes["hw"], axes["c_out"], axes["c_in"], axes["aux"])]
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv3_routes.json")
    got = record()
    tiles = sorted({t for row in got.values() for t in row})
    assert len(tiles) <= 10
    routes = {k: "".join(str(tiles.index(t)) for t in row) for k, row in got.items()}
    with open(path, "w") as f:
        json.dump(dict(axes=AXES, tiles=tiles, routes=routes), f, indent=0, sort_keys=True)
        f.write("\n")
    for mode in AXES["SSDE_WINOGRAD"]:
        print("SSDE_WINOGRAD=%s:" % mode, {t: sum(row.count(t) for k, row in got.items() if k.startswith(mode + "/")) for t in tiles})
