"""moped_amd/host/kinect_depthmap_test run for real: hipKinectDepthmap (KINECT_DEPTHMAP_HIP.hpp), the replacement for the
map-building block of moped3d's ROS node (moped3d/moped3d.cpp:270-333), against the program's own plain C++ loop on the
same raw buffer -- 0 differing bytes, for a raw buffer of the map's size and for one of half the size."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "moped_amd", "host", "kinect_depthmap_test")


def run(args):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    t = r.stdout.split()
    assert t[:1] == ["DIFF"] and t[2] == "OF" and t[4] == "INVALID", (r.returncode, r.stdout, r.stderr[-2000:])
    return r.returncode, int(t[1]), int(t[3]), int(t[5])


@pytest.mark.parametrize("fmt", ["f32", "u16", "cloud"])
@pytest.mark.parametrize("raw,size", [((640, 480), (640, 480)), ((320, 240), (640, 480)), ((33, 17), (66, 34)),
                                      ((32, 16), (70, 40))], ids=lambda v: "%dx%d" % v)
def test_helper_equals_the_host_loop(fmt, raw, size):
    rc, diff, total, invalid = run(["--format", fmt, "--raw", raw[0], raw[1], "--map", size[0], size[1]])
    assert total == size[0] * size[1] * 16
    assert 0 < invalid < size[0] * size[1]           # missing readings and valid pixels both
    assert diff == 0 and rc == 0, (diff, rc)
