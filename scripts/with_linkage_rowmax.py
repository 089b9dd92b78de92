#!/usr/bin/env python3
"""Runs another script of the repository with the linkage clusterer in MH_LINKAGE_ROWMAX mode, for A/B measurements of
scripts that do not know the mode (bench.py, scripts/kinect_image_bench.py): every context that is given the linkage
clusterer (capi.Context.frame_set_cluster_linkage) is switched to capi.LINKAGE_ROWMAX in the same call.  The library
itself reads no switch from the environment; this wrapper changes what the Python side asks for.

    python scripts/with_linkage_rowmax.py bench.py --gpus 1 --models 50 --depth-kind 1 --moped3d-frontend
    python scripts/with_linkage_rowmax.py scripts/kinect_image_bench.py"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moped_amd import capi  # noqa: E402

_set = capi.Context.frame_set_cluster_linkage


def _set_rowmax(self, params):
    _set(self, params)
    if params is not None:
        self.linkage_set_mode(capi.LINKAGE_ROWMAX)


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    capi.Context.frame_set_cluster_linkage = _set_rowmax
    script = sys.argv[1]
    sys.argv = sys.argv[1:]
    sys.path.insert(0, os.path.dirname(os.path.abspath(script)))
    print("[with_linkage_rowmax] CLUSTER_LINKAGE in MH_LINKAGE_ROWMAX mode", file=sys.stderr)
    runpy.run_path(script, run_name="__main__")


if __name__ == "__main__":
    main()
