"""The inputs of tests/test_gpu_wms_frame.py bite, shown on the CPU before the device is trusted: over the oracle's match
lists of frame 0 (tests/test_gpu_linkage_stages.py's 20-model frames and maps) the restatement of moped3d's weighted mean
shift gives overlapping clusters whose per-model members / matches ratio is inside MH_WMS_MEMBER_FACTOR for the cases that
must not be cut, exactly at it for one, and past it for the case built to be cut."""
import numpy as np

import orclib
import test_gpu_linkage_stages as ls
import test_gpu_wms_frame as tf
from moped_amd import synth


def _ratios(rows, mm):
    return {m: sum(len(r[1]) for r in rows if r[0] == m) / int((mm == m).sum()) for m in {r[0] for r in rows}}


def test_frame_cases_lie_where_the_gpu_tests_need_them():
    db = synth.make_db(ls.N_MODELS, 400, seed=11)
    dbn = orclib.normalize(db.desc)
    fr = ls.counted_frame(db, ls.PLANTED, 40)
    img, fill = ls.frame_maps(db, fr, 0)
    lists = ls.oracle_lists(db, dbn, fr, img, fill)
    mq = np.concatenate([l[0] for l in lists])
    mm = np.concatenate([np.full(len(l[0]), m, np.int32) for m, l in enumerate(lists)])
    for prm, lo, hi in ((tf.DEFAULT, 1.0, tf.FACTOR), (tf.OVERLAP, 2.0, tf.FACTOR), (tf.AT_FACTOR, tf.FACTOR, tf.FACTOR)):
        rows, begin, over = tf.restated(fr, img, fill, mq, mm, prm)
        top = max(_ratios(rows, mm).values())
        print(prm, len(rows), "rows, largest members / matches", top)
        assert not over and lo <= top <= hi and len(rows) >= 10, prm
    rows, begin, over = tf.restated(fr, img, fill, mq, mm, tf.EXCEED)
    assert len(over) >= 5 and max(_ratios(rows, mm).values()) <= tf.FACTOR
    for m in over:      # a cut model keeps whole clusters, and at least one
        assert any(r[0] == m for r in rows), m
