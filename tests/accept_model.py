"""What share of a frame's queries pass C can answer without a search (csrc/screen.h: screen_reject_proved), as a
host model: tests/test_screen_reject_cpu.py prints it, tests/test_gpu_accept_reject.py takes its floor from it.

The model sees float32 dot products in the place of the screen's f16 ones and no records: a query's largest value stands
for the largest upper bound, its THIRD largest for the second largest lower bound over distinct records (the best and the
second best row may share a record's block), and the threshold lies one margin below the second largest."""
import numpy as np

import orclib
from moped_amd import capi, synth


def reject_proved(qq, dmax, h1, l2, tau, ratio):
    f = np.float32
    return bool(capi.load().mh_screen_reject_proved(f(qq), f(dmax), f(h1), f(l2), f(tau), f(ratio)))


def top3_values(qn, dbn, dd, chunk=500, torch_dev=None):
    """The three largest w = dot(q, d) - dd / 2 of every query, descending, float32 arithmetic."""
    neg = (np.float32(-0.5) * dd).astype(np.float32)
    out = np.empty((len(qn), 3), np.float32)
    if torch_dev is not None:
        import torch
        tdb = torch.from_numpy(np.ascontiguousarray(dbn)).to(torch_dev)
        tneg = torch.from_numpy(neg).to(torch_dev)
    for i in range(0, len(qn), chunk):
        if torch_dev is not None:
            w = torch.from_numpy(np.ascontiguousarray(qn[i:i + chunk])).to(torch_dev) @ tdb.T + tneg[None, :]
            out[i:i + chunk] = torch.topk(w, 3, dim=1).values.cpu().numpy()
        else:
            w = qn[i:i + chunk] @ dbn.T + neg[None, :]
            out[i:i + chunk] = -np.partition(-w, 2, axis=1)[:, :3]
            out[i:i + chunk].sort(axis=1)
            out[i:i + chunk] = out[i:i + chunk][:, ::-1]
    return out


def predicted_share(qn, dbn, ratio, torch_dev=None):
    """Share of the queries `qn` (normalised rows) the model proves rejected at `ratio` against the rows `dbn`."""
    dd, qq = orclib.row_norms(dbn), orclib.row_norms(qn)
    dmax = float(np.sqrt(dd.max()))
    t3 = top3_values(qn, dbn, dd, torch_dev=torch_dev)
    L = capi.load()
    n = 0
    for i in range(len(qn)):
        tau = np.float32(t3[i, 1]) - np.float32(L.mh_screen_margin(np.float32(qq[i]), np.float32(dmax)))
        n += reject_proved(qq[i], dmax, t3[i, 0], t3[i, 2], tau, ratio)
    return n / len(qn)


def synth_frames(seeds=(0, 1, 2, 3), Q=3000):
    """The 20 x 5 000 DB and frames bench.py's workload is made of: (db, normalised rows, [normalised queries per seed])."""
    db = synth.make_db(20, 5000)
    dbn = orclib.normalize(db.desc)
    return db, dbn, [orclib.normalize(synth.make_frame(db, n_vis=2, seed=s, Q=Q).desc) for s in seeds]
