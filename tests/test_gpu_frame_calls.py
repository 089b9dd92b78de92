"""A frame call's parameters do not outlive the call.  One long-lived context goes through the entry points that hand
frame_rest a stride, an offset into the top-2 arrays, a result slot, a frame number, a stage range or a depth map of
their own -- strided and batched rest chains, merged batches and batches frame after frame, a stepped frame that is
abandoned, calls that are refused -- and after each of them a plain frame gives, bit for bit, what it gave at first;
and each of those calls gives, per slot, what it gives on a fresh context with the same DB."""
import numpy as np
import pytest

import group_ref as g
import orclib
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
Q, B, W = 256, 3, 2
PAD = np.int32(0x7FC0DEAD)   # what lies between the blocks of a strided exchange buffer: never a row, never a distance


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), (what, i)
        if a is not None:
            assert a.dtype == b.dtype and np.array_equal(_bytes(a), _bytes(b)), (what, i)


class World:
    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.db = synth.make_db(4, 400, seed=5)
        n = self.db.n
        dbn = orclib.normalize(self.db.desc)
        self.frames = [synth.make_frame(self.db, n_vis=2, seed=40 + f, Q=Q, pts_per_obj=60) for f in range(B + 1)]
        self.plain_frame = self.frames[B]
        self.prm = capi.default_frame_params()
        self.seeds = [7 + f for f in range(B)]
        # the shards' exchange-1 words of the B frames: shard s holds rows [s n / W, (s + 1) n / W)
        self.words = []
        for fr in self.frames[:B]:
            qn = orclib.normalize(fr.desc)
            idx_s, d1_s, d2_s = [], [], []
            for s in range(W):
                lo, hi = s * n // W, (s + 1) * n // W
                idx, d1, d2 = orclib.match_2nn(dbn[lo:hi], qn)
                idx_s.append(np.asarray(idx, np.int32) + lo)
                d1_s.append(d1)
                d2_s.append(d2)
            self.words.append(g.blocks(np.stack(idx_s), np.stack(d1_s).astype(np.float32), np.stack(d2_s).astype(np.float32)))

    def ctx(self, timing=False):
        c = capi.Context(0)
        c.db_upload(self.db.desc, self.db.model_of, self.db.xyz, self.db.n_models)
        c.reserve_batch(Q, B)
        if timing:
            c.enable_timing(True)
        return c

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    # ---- what a call leaves behind --------------------------------------------------------------------------------
    @staticmethod
    def single(c):
        objs, counts = c.frame_fetch()
        q, m = c.frame_fetch_matches()
        return [objs, counts, q, m, c.frame_fetch_match_reps(), c.frame_fetch_match_points()]

    @staticmethod
    def slots(c):
        out = []
        for f in range(B):
            objs, counts = c.frame_fetch_slot(f)
            out += [objs, counts]
            try:    # (frames that went through the stages one after the other: only the last one's lists remain)
                q, m = c.frame_fetch_matches_slot(f)
                out += [q, m, c.frame_fetch_match_reps(f)]
            except capi.MhError:
                out += [None, None, None]
        return out

    # ---- the calls ------------------------------------------------------------------------------------------------
    def plain(self, c):
        fr = self.plain_frame
        d, u = self.up(fr.desc), self.up(fr.uv)
        c.frame_enqueue(d.data_ptr(), u.data_ptr(), Q, K, CAM0, self.prm, 3)
        return self.single(c)

    def rest_strided(self, c):
        stride = 3 * Q + 64
        buf = np.full(W * stride, PAD, np.int32)
        for s in range(W):
            buf[s * stride:s * stride + 3 * Q] = self.words[0][s].reshape(-1)
        w, u = self.up(buf), self.up(self.frames[0].uv)
        c.frame_enqueue_rest_strided(u.data_ptr(), Q, w.data_ptr(), W, stride, K, CAM0, self.prm, self.seeds[0])
        return self.single(c)

    def batch(self, c):
        d = self.up(np.concatenate([fr.desc for fr in self.frames[:B]]))
        u = self.up(np.concatenate([fr.uv for fr in self.frames[:B]]))
        c.frame_enqueue_batch(d.data_ptr(), u.data_ptr(), Q, B, K, CAM0, self.prm, self.seeds)
        return self.slots(c)

    def rest_frames(self, c):
        plane = B * Q + 32
        stride = 3 * plane
        buf = np.full(W * stride, PAD, np.int32)
        for s in range(W):
            for k in range(3):
                for f in range(B):
                    at = s * stride + k * plane + f * Q
                    buf[at:at + Q] = self.words[f][s, k]
        w = self.up(buf)
        u = self.up(np.concatenate([fr.uv for fr in self.frames[:B]]))
        c.frame_enqueue_rest_frames(u.data_ptr(), Q, w.data_ptr(), W, stride, plane, B, K, CAM0, self.prm, self.seeds)
        return self.slots(c)

    def fresh(self, call, timing=False):
        c = self.ctx(timing)
        try:
            return call(c)
        finally:
            c.close()


@pytest.fixture(scope="module")
def world():
    return World()


def test_call_parameters_do_not_outlive_the_call(world):
    w = world
    c = w.ctx()
    try:
        first = w.plain(c)                                   # 1
        assert len(first[0]) >= 1 and first[1][0] > 50 and first[1][1] >= 1   # objects, matches and clusters to compare
        for name, call in (("rest_strided", w.rest_strided), ("batch", w.batch), ("rest_frames", w.rest_frames)):   # 2 - 4
            got = call(c)
            _same(got, w.fresh(call), name)
            assert any(len(o) for o in ([got[0]] if name == "rest_strided" else got[0::5])), name   # (objects to compare)
            _same(w.plain(c), first, "plain after " + name)
        # 5: the same batches frame after frame (stage timing keeps the frames of a batch apart)
        c.enable_timing(True)
        for name, call in (("batch", w.batch), ("rest_frames", w.rest_frames)):
            got = call(c)
            assert got[2] is None and got[-1] is not None, name   # (only the last frame's lists remain: the loop ran)
            _same(got, w.fresh(call, timing=True), name + ", frame after frame")
            c.enable_timing(False)
            _same(w.plain(c), first, "plain after " + name + ", frame after frame")
            c.enable_timing(True)
        c.enable_timing(False)
        # 6: a stepped frame, abandoned after CLUSTER
        fr = w.frames[1]
        off, mq, _ = c.step_match(fr.desc.copy(), fr.uv, K, CAM0)
        assert off[-1] == len(mq) > 50
        cl_model, _, _ = c.step_cluster()
        assert len(cl_model) >= 1
        _same(w.plain(c), first, "plain after an abandoned stepped frame")
        # 7: refused calls change nothing
        before = w.single(c)
        u, wd = w.up(w.frames[0].uv), w.up(np.full(W * 3 * (B * Q + 32), PAD, np.int32))
        with pytest.raises(capi.MhError, match="-> -1"):     # MH_ERR_ARG
            c.frame_enqueue_rest_strided(u.data_ptr(), Q, wd.data_ptr(), W, 3 * Q - 1, K, CAM0, w.prm, 1)
        with pytest.raises(capi.MhError, match="-> -1"):
            c.frame_enqueue_rest_batch(u.data_ptr(), Q, wd.data_ptr(), W, 3 * (B * Q + 32), B * Q + 32, capi.MAX_BATCH,
                                       K, CAM0, w.prm, 1)
        _same(w.single(c), before, "fetch after the refused calls")
        _same(w.plain(c), first, "plain after the refused calls")   # 8
    finally:
        c.close()
