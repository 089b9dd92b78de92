"""Frame driver over the C ABI: device-resident MATCH -> CLUSTER -> POSE -> FILTER ->
POSE2 -> FILTER2, one mh_ctx per frame in flight, optional model sharding over
ranks with the two small exchanges of SURVEY.md 8(e).

PyTorch is used for what the C ABI does not own: device buffers for the frame
inputs, HIP streams, and handing rank 0's communicator id to the other ranks.  All
computation AND the exchanges (ncclAllGather on the slot's stream, csrc/comm.hip)
happen inside libmoped_hip.so.
"""
from __future__ import annotations

import os as _os
# one hardware queue per frame slot: ROCm's default of 4 caps the overlap of the slots' streams at four kernels (image ->
# objects: 1 540 -> 2 920 frames/s with 16).  Read by the HIP runtime when it creates its queues, so this only helps if the
# process has not touched the GPU yet; a C++ host exports it before it starts.
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

import numpy as np
import torch

from . import capi


def models_of_rank(n_models: int, rank: int, world: int, assign: str = "block"):
    """Models rank `rank` of `world` owns: contiguous blocks [r n/W, (r+1) n/W), or round-robin (m % W == r --
    SURVEY.md 8(e): interleaving spreads the visible models' CLUSTER / POSE work over the ranks)."""
    if assign == "round-robin":
        return np.arange(rank, n_models, world, dtype=np.int64)
    if assign != "block":
        raise ValueError(f"unknown model assignment {assign!r}")
    return np.arange((rank * n_models) // world, ((rank + 1) * n_models) // world, dtype=np.int64)


class ShardedDB:
    """This rank's slice of the model database.  Rows of a model are contiguous in the flattened DB
    (MATCH_ANN_CPU::Update order), so a shard is a list of runs of global rows, in ascending order: ONE run for the
    block assignment (`row_lo` = mh_db_upload's index_base), one per maximal run of owned models for round-robin
    (mh_db_upload_blocks).  Row and model ids stay global either way."""

    def __init__(self, desc, xyz, model_of, n_models, rank=0, world=1, assign="block"):
        model_of = np.asarray(model_of, np.int32)
        owned = np.zeros(n_models + 1, bool)
        owned[models_of_rank(n_models, rank, world, assign)] = True
        mine = owned[model_of]
        rows = np.nonzero(mine)[0]
        # maximal runs of consecutive global rows
        starts = rows[np.r_[True, np.diff(rows) != 1]] if len(rows) else np.zeros(0, np.int64)
        ends = rows[np.r_[np.diff(rows) != 1, True]] + 1 if len(rows) else np.zeros(0, np.int64)
        self.block_global_row = starts.astype(np.int32)
        self.block_rows = (ends - starts).astype(np.int32)
        self.rows = rows.astype(np.int32)   # global row of every local row
        self.row_lo = int(rows[0]) if len(rows) else 0
        self.row_hi = int(rows[-1]) + 1 if len(rows) else 0
        self.desc = np.ascontiguousarray(desc[rows], np.float32)
        self.xyz = np.ascontiguousarray(xyz[rows], np.float32)
        self.model_of = np.ascontiguousarray(model_of[rows])
        self.n_models = n_models          # model ids stay global
        self.rank, self.world, self.assign = rank, world, assign
        self.views = np.ones(len(rows), np.int32)   # per row: the views that saw it (merge_kinect_view counts; else 1)

    def splice(self, op: int, model: int, desc=None, xyz=None):
        """Keeps the host arrays in step with an edit of the resident store (Context.db_splice): model `model` inserted,
        replaced or removed, later models renumbered.  One rank only: a sharded store is not editable."""
        if self.world > 1 or len(self.block_rows) > 1 or self.row_lo != 0:
            raise ValueError("a sharded model database cannot be edited in place")
        if op == capi.DB_INSERT:
            b = e = int(np.searchsorted(self.model_of, model, "left"))
        else:
            b, e = (int(np.searchsorted(self.model_of, model, side)) for side in ("left", "right"))
        if op == capi.DB_REMOVE:
            desc, xyz = np.zeros((0, 128), np.float32), np.zeros((0, 3), np.float32)
        desc = np.ascontiguousarray(desc, np.float32).reshape(-1, 128)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        delta = {capi.DB_INSERT: 1, capi.DB_REPLACE: 0, capi.DB_REMOVE: -1}[op]
        self.desc = np.ascontiguousarray(np.concatenate([self.desc[:b], desc, self.desc[e:]]))
        self.xyz = np.ascontiguousarray(np.concatenate([self.xyz[:b], xyz, self.xyz[e:]]))
        self.model_of = np.concatenate([self.model_of[:b], np.full(len(desc), model, np.int32),
                                        self.model_of[e:] + np.int32(delta)]).astype(np.int32)
        self.views = np.concatenate([self.views[:b], np.ones(len(desc), np.int32), self.views[e:]]).astype(np.int32)
        self.n_models += delta
        n = len(self.model_of)
        self.rows = np.arange(n, dtype=np.int32)
        self.row_lo, self.row_hi = 0, n
        self.block_global_row = np.zeros(1 if n else 0, np.int32)
        self.block_rows = np.full(1 if n else 0, n, np.int32)

    def append(self, model: int, desc, xyz):
        """The append form of `splice` (Context.db_append): rows behind the last row of an existing model; the model
        keeps its index, the model ids stay as they are."""
        if not 0 <= model < self.n_models:
            raise ValueError("model index out of range")
        if self.world > 1 or len(self.block_rows) > 1 or self.row_lo != 0:
            raise ValueError("a sharded model database cannot be edited in place")
        e = int(np.searchsorted(self.model_of, model, "right"))
        desc = np.ascontiguousarray(desc, np.float32).reshape(-1, 128)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self.desc = np.ascontiguousarray(np.concatenate([self.desc[:e], desc, self.desc[e:]]))
        self.xyz = np.ascontiguousarray(np.concatenate([self.xyz[:e], xyz, self.xyz[e:]]))
        self.model_of = np.concatenate([self.model_of[:e], np.full(len(desc), model, np.int32), self.model_of[e:]]).astype(np.int32)
        self.views = np.concatenate([self.views[:e], np.ones(len(desc), np.int32), self.views[e:]]).astype(np.int32)
        n = len(self.model_of)
        self.rows = np.arange(n, dtype=np.int32)
        self.row_lo, self.row_hi = 0, n
        self.block_global_row = np.zeros(1 if n else 0, np.int32)
        self.block_rows = np.full(1 if n else 0, n, np.int32)

    def patch(self, model: int, idx, desc, xyz, views=None):
        """Rows `idx` (relative to the model's first row) of an existing model overwritten (Context.db_merge_view's
        merged rows: raw sums and points); views: the model's counts after the edit, for all its rows."""
        if not 0 <= model < self.n_models:
            raise ValueError("model index out of range")
        if self.world > 1 or len(self.block_rows) > 1 or self.row_lo != 0:
            raise ValueError("a sharded model database cannot be edited in place")
        b, e = (int(np.searchsorted(self.model_of, model, side)) for side in ("left", "right"))
        idx = np.asarray(idx, np.int64).reshape(-1)
        if len(idx) and (idx.min() < 0 or idx.max() >= e - b):
            raise ValueError("a row outside the model")
        self.desc[b + idx] = np.asarray(desc, np.float32).reshape(-1, 128)
        self.xyz[b + idx] = np.asarray(xyz, np.float32).reshape(-1, 3)
        if views is not None:
            self.views[b:e] = np.asarray(views, np.int32).reshape(e - b)

    def keep(self, model: int, mask):
        """An existing model keeps the rows whose flag is set, in order (Context.db_keep_rows)."""
        if not 0 <= model < self.n_models:
            raise ValueError("model index out of range")
        if self.world > 1 or len(self.block_rows) > 1 or self.row_lo != 0:
            raise ValueError("a sharded model database cannot be edited in place")
        b, e = (int(np.searchsorted(self.model_of, model, side)) for side in ("left", "right"))
        mask = np.asarray(mask).reshape(-1) != 0
        if len(mask) != e - b:
            raise ValueError("one flag per row of the model")
        stay = np.ones(len(self.model_of), bool)
        stay[b:e] = mask
        self.desc = np.ascontiguousarray(self.desc[stay])
        self.xyz = np.ascontiguousarray(self.xyz[stay])
        self.model_of = np.ascontiguousarray(self.model_of[stay])
        self.views = np.ascontiguousarray(self.views[stay])
        n = len(self.model_of)
        self.rows = np.arange(n, dtype=np.int32)
        self.row_lo, self.row_hi = 0, n
        self.block_global_row = np.zeros(1 if n else 0, np.int32)
        self.block_rows = np.full(1 if n else 0, n, np.int32)

    def upload(self, ctx: "capi.Context", normalized):
        if len(self.block_rows) > 1:
            ctx.db_upload_blocks(normalized, self.model_of, self.xyz, self.n_models, self.block_global_row, self.block_rows)
        else:
            ctx.db_upload(normalized, self.model_of, self.xyz, self.n_models, index_base=self.row_lo)


class FramePipeline:
    """`depth` frames in flight on one GPU; each has its own mh_ctx + HIP stream so
    the latency-bound CLUSTER/POSE/FILTER kernels of one frame overlap the MATCH
    kernel of the next.

    With a sharded DB (world > 1, or force_exchange to run the same code on one rank) every frame goes through
    mh_frame_enqueue_sharded[_batch]: the exchanges happen inside libmoped_hip.so, on the slot's stream, over
    communicators this class only creates --
      * RCCL (mh_comm_create) when torch.distributed runs on nccl or is not initialised (world 1): rank 0's id
        travels by broadcast_object_list; `n_comms` communicators, slot i uses communicator i % n_comms;
      * the host transport (mh_comm_create_host over the gloo group) when the group is gloo: ranks that share one
        device (RCCL refuses that), the rehearsal of tests/test_gpu_dist.py."""

    def __init__(self, device: int, db: ShardedDB, depth: int = 1, max_queries: int = 4096,
                 params: capi.mh_frame_params | None = None, K=None, cam=None, group=None,
                 force_exchange: bool = False, n_comms: int = 4, batch: int = 1, lane: "tuple | None" = None,
                 id_leader: "int | None" = None, db_capacity: "tuple | None" = None):
        from . import synth
        self.dev = torch.device(f"cuda:{device}")
        torch.cuda.set_device(self.dev)
        self.db = db
        self.params = params or capi.default_frame_params()
        self.K = synth.K_DEFAULT if K is None else K
        self.cam = synth.CAM_IDENTITY if cam is None else cam
        self.group = group
        # A models x frames grid (bench.py --parallelism grid): this pipeline's communicators span the db.world ranks of ONE
        # frame group.  `id_leader` = the rank (of the default process group) that is shard 0 of this rank's frame group: the
        # RCCL ids then travel by ONE all_gather_object over the default group per communicator, which every rank of the
        # job joins -- no torch-side NCCL communicator per frame group.  `group` (a gloo subgroup of the frame group's ranks)
        # carries the host transport of the rehearsal instead.
        self.id_leader = id_leader
        self.world = db.world
        self.ctxs, self.streams = [], []
        normalized = None
        for i in range(depth):
            c = capi.Context(device)
            s = torch.cuda.Stream(device=self.dev)
            c.set_stream(s.cuda_stream)   # before any work: the context then never creates a stream of its own
            if i == 0:
                # model descriptors are L2-normalised once, like Update() (MATCH_ANN_CPU.hpp:94)
                normalized = c.normalize(db.desc) if db.desc.shape[0] else db.desc
                db.upload(c, normalized)
                if db_capacity:   # (max_rows, max_models): edits inside it allocate nothing (mh_db_reserve)
                    c.db_reserve(*db_capacity)
            else:
                c.db_share(self.ctxs[0])   # one store per GPU: every frame in flight searches the same copy
            if batch > 1:   # frames travel in batches: per-frame working arrays, `batch` copies (mh_reserve_batch)
                c.reserve_batch(-(-max_queries // batch), batch)
            else:
                c.reserve(max_queries)
            self.ctxs.append(c)
            self.streams.append(s)
        self.depth = depth
        self.model_names = [None] * db.n_models   # add_model(name=...): a known name replaces, like Moped::addModel
        # lane = (n_streams, reserve_cus_per_xcd, low_priority): the contexts' chip-filling MATCH passes on shared streams
        self.lane = None
        if lane:
            self.lane = capi.Lane(device, *lane)
            for c in self.ctxs:
                c.set_lane(self.lane)
        self.exchange = force_exchange or self.world > 1
        self.comms = []
        if self.exchange:
            self.comms = self._make_comms(max(1, min(n_comms, depth)))
        self._batch = [1] * depth
        self._inputs = [None] * depth   # the slot's current input tensors: its stream may still be reading them
        self._raw_maps = [None] * depth   # enqueue_kinect_raw_batch: the slot's (depth maps, distance maps), flat, grown on demand
        self._cam = capi.make_cam(self.K, self.cam)

    def _make_comms(self, n):
        import torch.distributed as dist
        inited = dist.is_available() and dist.is_initialized()
        if inited and dist.get_backend(self.group) == "gloo":
            def allgather(blob: bytes) -> bytes:
                mine = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
                out = torch.empty(self.world * mine.numel(), dtype=torch.uint8)
                dist.all_gather_into_tensor(out, mine, group=self.group)
                return out.numpy().tobytes()
            return [capi.Comm.create_host(self.ctxs[0], self.db.rank, self.world, allgather)]
        comms = []
        for _ in range(n):
            ids = [capi.comm_unique_id() if self.db.rank == 0 else None]
            if self.id_leader is not None and inited:
                every = [None] * dist.get_world_size()
                dist.all_gather_object(every, ids[0])
                ids[0] = every[self.id_leader]
            elif self.world > 1:
                src = 0 if self.group is None else dist.get_global_rank(self.group, 0)
                dist.broadcast_object_list(ids, src=src, group=self.group)
            comms.append(capi.Comm.create(self.ctxs[0], ids[0], self.db.rank, self.world))
        return comms

    def _comm(self, slot):
        return self.comms[slot % len(self.comms)]

    def comm_info(self):
        """What carries the frames' exchange: (rank, world, transport) of this rank's communicators."""
        if not self.comms:
            return None
        r, w, rccl = self.comms[0].info()
        return {"rank": r, "world": w, "transport": "RCCL ncclAllGather" if rccl else "host callback (gloo)",
                "communicators": len(self.comms)}

    # ---- the model set while frames flow: Moped::addModel / removeModel (moped.cpp:139-159) ---------------
    def _edit(self, op, model, desc=None, xyz=None):
        """One splice on slot 0's context, stream ordered; the other slots adopt the new store behind their frames in
        flight.  No stream is synchronised: frames already enqueued finish on the store they were enqueued against."""
        if self.world > 1 or self.exchange:
            raise ValueError("a sharded model database cannot be edited in place: rebuild the pipeline")
        self.ctxs[0].db_splice(op, model, desc, xyz, normalize=True)   # raw rows, normalised on the device like Update()
        for c in self.ctxs[1:]:
            c.db_adopt(self.ctxs[0])
        self.db.splice(op, model, desc, xyz)

    def add_model(self, desc, xyz, name=None) -> int:
        """desc [n,128] raw descriptors, xyz [n,3].  A new model is appended; a name already known replaces that model
        and keeps its index (moped.cpp:141-144).  Returns the model's index."""
        if name is not None and name in self.model_names:
            i = self.model_names.index(name)
            self._edit(capi.DB_REPLACE, i, desc, xyz)
            return i
        i = self.db.n_models
        self._edit(capi.DB_INSERT, i, desc, xyz)
        self.model_names.append(name)
        return i

    def replace_model(self, i: int, desc, xyz):
        self._edit(capi.DB_REPLACE, i, desc, xyz)

    def remove_model(self, i: int):
        """Later models move down by one (removeModel erases from the vector, moped.cpp:152-159)."""
        self._edit(capi.DB_REMOVE, i)
        del self.model_names[i]

    # ---- a model taught from a device image: Moped::createPlanarModelsFromImages (moped.cpp:196-236) ----------
    def _adopt_planar(self, op, i, desc, xyz):
        for c in self.ctxs[1:]:
            c.db_adopt(self.ctxs[0])
        self.db.splice(op, i, desc, xyz)

    def _warn_if_truncated(self, max_keypoints):
        if self.ctxs[0].planar_truncated:   # MH_ERR_CAPACITY: the edit is made, from the first keypoints of the list
            import warnings
            warnings.warn(f"an image has more keypoints than max_keypoints={max_keypoints}: its model holds the first "
                          f"{max_keypoints} of FEAT's list", RuntimeWarning, stacklevel=3)

    def add_planar_model(self, image_dev: torch.Tensor, name=None, scale=None, z=None, roi=None, max_rows=0,
                         max_keypoints: int = 4096, double_size: bool = True):
        """image_dev [h, w] uint8 on this GPU -> a model of the resident store whose points are the image's keypoints:
        at (u scale, v scale, 0) with `scale` (the reference's form), or on the plane at depth `z` in front of the
        pipeline's camera K with `z`; exactly one of the two.  roi = (u0, v0, u1, v1) keeps the keypoints inside it,
        max_rows the first so many.  FEAT, the selection and the splice run on slot 0's stream, the other slots adopt;
        the rows do not leave the device for the edit (a host copy keeps `self.db` in step).  A known name replaces that
        model.  An image with more keypoints than max_keypoints is taught from the first max_keypoints of FEAT's list and
        a RuntimeWarning says so.  Returns (index, n_rows, bbox[6])."""
        if self.world > 1 or self.exchange:
            raise ValueError("a sharded model database cannot be edited in place: rebuild the pipeline")
        spec = capi.make_planar_spec(scale=scale, z=z, K=self.K, roi=roi, max_rows=max_rows)
        h, w = image_dev.shape
        known = name is not None and name in self.model_names
        i = self.model_names.index(name) if known else self.db.n_models
        op = capi.DB_REPLACE if known else capi.DB_INSERT
        n, bbox, desc, xyz = self.ctxs[0].db_splice_image(op, i, image_dev.data_ptr(), w, h, spec, double_size,
                                                          max_keypoints, want_rows=True)
        self._adopt_planar(op, i, desc, xyz)
        self._warn_if_truncated(max_keypoints)
        if not known:
            self.model_names.append(name)
        return i, n, bbox

    def add_planar_models(self, images_dev, names, scale=None, z=None, roi=None, max_rows=0, max_keypoints: int = 4096,
                          double_size: bool = True):
        """The same for several images of one size: new names through ONE FEAT batch and one selection launch
        (mh_db_splice_images), known names one by one.  Returns a list of (index, n_rows, bbox)."""
        if self.world > 1 or self.exchange:
            raise ValueError("a sharded model database cannot be edited in place: rebuild the pipeline")
        if len(images_dev) != len(names):
            raise ValueError("one name per image")
        out = [None] * len(names)
        fresh = [k for k, nm in enumerate(names) if nm is None or (nm not in self.model_names and nm not in names[:k])]
        for b in range(0, len(fresh), capi.MAX_BATCH):
            part = fresh[b:b + capi.MAX_BATCH]
            spec = capi.make_planar_spec(scale=scale, z=z, K=self.K, roi=roi, max_rows=max_rows)
            h, w = images_dev[part[0]].shape
            if any(tuple(images_dev[k].shape) != (h, w) for k in part):
                raise ValueError("the images of one call have one size")
            first = self.db.n_models
            n, bbox, desc, xyz = self.ctxs[0].db_splice_images(first, [images_dev[k].data_ptr() for k in part], w, h, spec,
                                                               double_size, max_keypoints, want_rows=True)
            for c in self.ctxs[1:]:
                c.db_adopt(self.ctxs[0])
            self._warn_if_truncated(max_keypoints)
            for j, k in enumerate(part):
                self.db.splice(capi.DB_INSERT, first + j, desc[j], xyz[j])
                self.model_names.append(names[k])
                out[k] = (first + j, int(n[j]), bbox[j])
        for k, nm in enumerate(names):   # known names (or a name given twice) replace, as addModel does
            if k not in fresh:
                out[k] = self.add_planar_model(images_dev[k], nm, scale, z, roi, max_rows, max_keypoints, double_size)
        return out

    # ---- a 3-D model taught from Kinect views: image + depth map + the object's pose in the view ------------------
    def _view_args(self, depth_dev, fill_dev, pose, roi, box, max_fill_distance, max_rows, merge_ratio=0.0, merge_dist=-1.0):
        if self.world > 1 or self.exchange:
            raise ValueError("a sharded model database cannot be edited in place: rebuild the pipeline")
        view = capi.make_view(depth_dev.data_ptr(), fill_dev.data_ptr() if fill_dev is not None else None, pose, self.K)
        spec = capi.make_view_spec(roi=roi, box=box, max_fill_distance=max_fill_distance, max_rows=max_rows,
                                   merge_ratio=merge_ratio, merge_dist=merge_dist)
        return view, spec

    def add_kinect_model(self, image_dev: torch.Tensor, depth_dev: torch.Tensor, fill_dev=None, name=None, pose=None,
                         roi=None, box=None, max_fill_distance=-1.0, max_rows=0, max_keypoints: int = 4096,
                         double_size: bool = True):
        """image_dev [h, w] uint8, depth_dev [h, w, 4] float32 (the map every depth entry point takes), optionally
        fill_dev [h, w], all on this GPU -> a model whose points are the measured 3-D points of the image's keypoints,
        in the model frame: pose = (qx, qy, qz, qw, tx, ty, tz) is the object's pose in this view, X_cam = R X_model + t
        (None = the camera frame is the model frame).  roi / box / max_fill_distance / max_rows: mh_view_spec.  A known
        name replaces that model.  FEAT, the selection and the splice run on slot 0's stream, the other slots adopt; a
        host copy of the rows keeps `self.db` in step.  Returns (index, n_rows, bbox[6], stats[8]); the caller
        refreshes moped3d's control points from bbox / n_rows, as after add_model."""
        view, spec = self._view_args(depth_dev, fill_dev, pose, roi, box, max_fill_distance, max_rows)
        h, w = image_dev.shape
        known = name is not None and name in self.model_names
        i = self.model_names.index(name) if known else self.db.n_models
        op = capi.DB_REPLACE if known else capi.DB_INSERT
        n, bbox, stats, desc, xyz = self.ctxs[0].db_splice_view(op, i, image_dev.data_ptr(), view, w, h, spec, double_size,
                                                               max_keypoints, want_rows=True)
        self._adopt_planar(op, i, desc, xyz)
        self._warn_if_truncated(max_keypoints)
        if not known:
            self.model_names.append(name)
        return i, n, bbox, stats

    def add_kinect_models(self, images_dev, depths_dev, names, fills_dev=None, poses=None, roi=None, box=None,
                          max_fill_distance=-1.0, max_rows=0, max_keypoints: int = 4096, double_size: bool = True):
        """The same for several views of one size, each a model of its own: new names through ONE FEAT batch and one
        selection launch (mh_db_splice_views), known names one by one.  Duplicates among the views are not looked for.
        Returns a list of (index, n_rows, bbox, stats); control points as after add_kinect_model."""
        if not (len(images_dev) == len(depths_dev) == len(names)):
            raise ValueError("one depth map and one name per image")
        fills_dev = fills_dev if fills_dev is not None else [None] * len(names)
        poses = poses if poses is not None else [None] * len(names)
        out = [None] * len(names)
        fresh = [k for k, nm in enumerate(names) if nm is None or (nm not in self.model_names and nm not in names[:k])]
        for b in range(0, len(fresh), capi.MAX_BATCH):
            part = fresh[b:b + capi.MAX_BATCH]
            h, w = images_dev[part[0]].shape
            if any(tuple(images_dev[k].shape) != (h, w) for k in part):
                raise ValueError("the images of one call have one size")
            views = []
            for k in part:
                view, spec = self._view_args(depths_dev[k], fills_dev[k], poses[k], roi, box, max_fill_distance, max_rows)
                views.append(view)
            first = self.db.n_models
            n, bbox, stats, desc, xyz = self.ctxs[0].db_splice_views(first, [images_dev[k].data_ptr() for k in part], views, w, h,
                                                                    spec, double_size, max_keypoints, want_rows=True)
            for c in self.ctxs[1:]:
                c.db_adopt(self.ctxs[0])
            self._warn_if_truncated(max_keypoints)
            for j, k in enumerate(part):
                self.db.splice(capi.DB_INSERT, first + j, desc[j], xyz[j])
                self.model_names.append(names[k])
                out[k] = (first + j, int(n[j]), bbox[j], stats[j])
        for k, nm in enumerate(names):   # known names (or a name given twice) replace, as addModel does
            if k not in fresh:
                out[k] = self.add_kinect_model(images_dev[k], depths_dev[k], fills_dev[k], nm, poses[k], roi, box,
                                               max_fill_distance, max_rows, max_keypoints, double_size)
        return out

    def extend_kinect_model(self, i: int, image_dev: torch.Tensor, depth_dev: torch.Tensor, fill_dev=None, pose=None, roi=None,
                            box=None, max_fill_distance=-1.0, max_rows=0, merge_ratio=0.8, merge_dist=0.002,
                            max_keypoints: int = 4096, double_size: bool = True):
        """A further view of model i: its keypoints are appended behind the model's rows, except those the model holds
        already -- the ones MATCH accepts at merge_ratio whose nearest row is a row of model i within merge_dist (model
        units) of the keypoint's point.  merge_ratio <= 0 or merge_dist < 0: no such test, and no MATCH.  Returns
        (index, rows added, bbox of the whole model, stats[8]); the caller refreshes moped3d's control points from
        bbox and the model's new row count, as after add_model."""
        view, spec = self._view_args(depth_dev, fill_dev, pose, roi, box, max_fill_distance, max_rows, merge_ratio, merge_dist)
        h, w = image_dev.shape
        n, bbox, stats, desc, xyz = self.ctxs[0].db_append_view(i, image_dev.data_ptr(), view, w, h, spec, double_size,
                                                               max_keypoints, want_rows=True)
        for c in self.ctxs[1:]:
            c.db_adopt(self.ctxs[0])
        self.db.append(i, desc, xyz)
        self._warn_if_truncated(max_keypoints)
        return i, n, bbox, stats

    def merge_kinect_view(self, i: int, image_dev: torch.Tensor, depth_dev: torch.Tensor, fill_dev=None, pose=None, roi=None,
                          box=None, max_fill_distance=-1.0, max_rows=0, merge_ratio=0.8, merge_dist=0.002,
                          max_keypoints: int = 4096, double_size: bool = True):
        """A further view of model i, as extend_kinect_model, but the keypoints the model holds already are folded into the
        rows they re-observe (Context.db_merge_view): the row's descriptor and point become the mean over its views, its
        view count grows by one.  New rows count 1.  Returns (index, rows added, rows merged, bbox of the whole model,
        stats[8]); model_views(i) has the counts; prune_model drops the rows few views saw."""
        view, spec = self._view_args(depth_dev, fill_dev, pose, roi, box, max_fill_distance, max_rows, merge_ratio, merge_dist)
        h, w = image_dev.shape
        n, m, bbox, stats, views, midx, mdesc, mxyz, desc, xyz = self.ctxs[0].db_merge_view(
            i, image_dev.data_ptr(), view, w, h, spec, double_size, max_keypoints, views_in=self.model_views(i), want_rows=True)
        for c in self.ctxs[1:]:
            c.db_adopt(self.ctxs[0])
        self.db.patch(i, midx, mdesc, mxyz)
        self.db.append(i, desc, xyz)
        self.db.views[self.db.model_of == i] = views
        self._warn_if_truncated(max_keypoints)
        return i, n, m, bbox, stats

    def model_views(self, i: int) -> np.ndarray:
        """Per row of model i: how many views saw it (1 for rows that did not come through merge_kinect_view)."""
        if not 0 <= i < self.db.n_models:
            raise ValueError("model index out of range")
        return self.db.views[self.db.model_of == i].copy()

    def prune_model(self, i: int, min_views: int):
        """Model i keeps the rows at least min_views views saw (Context.db_keep_rows: a compaction on the device, no
        row is normalised again).  Returns (index, rows kept, bbox[6])."""
        if self.world > 1 or self.exchange:
            raise ValueError("a sharded model database cannot be edited in place: rebuild the pipeline")
        mask = self.model_views(i) >= int(min_views)
        n, bbox = self.ctxs[0].db_keep_rows(i, mask)
        for c in self.ctxs[1:]:
            c.db_adopt(self.ctxs[0])
        self.db.keep(i, mask)
        return i, n, bbox

    def append_model_rows(self, i: int, desc, xyz):
        """desc [n,128] raw descriptors, xyz [n,3] behind the last row of model i (Context.db_append), normalised on the
        device like Update(); stream ordered as every edit.  Returns (index, rows added, bbox of the whole model, None);
        control points as after add_model."""
        if self.world > 1 or self.exchange:
            raise ValueError("a sharded model database cannot be edited in place: rebuild the pipeline")
        self.ctxs[0].db_append(i, desc, xyz, normalize=True)
        for c in self.ctxs[1:]:
            c.db_adopt(self.ctxs[0])
        self.db.append(i, desc, xyz)
        mine = self.db.xyz[self.db.model_of == i]
        bbox = np.concatenate([mine.min(0), mine.max(0)]).astype(np.float32) if len(mine) else None
        return i, len(np.asarray(desc).reshape(-1, 128)), bbox, None

    # ---- single frame in slot i ------------------------------------------------------
    def enqueue(self, slot: int, q_desc: torch.Tensor, q_uv: torch.Tensor, seed: int = 1,
                after: "torch.cuda.Stream | None" = None):
        """q_desc [Q,128] float32 (normalised in place), q_uv [Q,2]; both on this GPU.
        Returns immediately; work is on the slot's stream.  `after`: a stream whose
        pending work produces the inputs (omit when they are already resident --
        waiting on the legacy default stream serialises every frame behind it)."""
        c, s = self.ctxs[slot], self.streams[slot]
        Q = q_desc.shape[0]
        self._inputs[slot] = (q_desc, q_uv)   # kept until the slot's next enqueue (stream order: the old ones are done by then)
        if after is not None:
            s.wait_stream(after)
        self._batch[slot] = 1
        if not self.exchange:
            c.frame_enqueue(q_desc.data_ptr(), q_uv.data_ptr(), Q, self.K, self.cam, self.params, seed)
            return
        c.frame_enqueue_sharded(self._comm(slot), q_desc.data_ptr(), q_uv.data_ptr(), Q, self.K, self.cam, self.params,
                                seed, _cam_struct=self._cam)

    # ---- batches of frames (small shards) ----------------------------------------------------
    def enqueue_batch(self, slot: int, q_desc: torch.Tensor, q_uv: torch.Tensor, B: int, seeds):
        """B frames through ONE MATCH launch and ONE exchange (a shard of a few thousand rows does not
        fill the chip for the 3000 queries of one frame): q_desc [B*Q,128], q_uv [B*Q,2], the frames one
        after the other; their CLUSTER..FILTER2 run one after the other on the slot's stream and leave
        their objects in result slots 0..B-1.  With a sharded DB through the exchange, otherwise
        mh_frame_enqueue_batch."""
        assert 1 <= B <= capi.MAX_BATCH
        c = self.ctxs[slot]
        self._inputs[slot] = (q_desc, q_uv)
        self._batch[slot] = B
        Q = q_desc.shape[0] // B
        if not self.exchange:
            c.frame_enqueue_batch(q_desc.data_ptr(), q_uv.data_ptr(), Q, B, self.K, self.cam, self.params, seeds,
                                  _cam_struct=self._cam)
            return
        c.frame_enqueue_sharded_batch(self._comm(slot), q_desc.data_ptr(), q_uv.data_ptr(), Q, B, self.K, self.cam,
                                      self.params, seeds, _cam_struct=self._cam)

    # ---- frames with several cameras from device images ------------------------------------------
    def enqueue_images(self, slot: int, gray_ptrs, w: int, h: int, Ks, cams, seed: int = 1, max_keypoints: int = 2048,
                       double_size: bool = True, keep=None):
        """ONE frame seen by len(gray_ptrs) cameras (Ks [n,4], cams [n,7]): 8-bit device images of one size in, objects
        out (fetch), the keypoint counts never leave the device.  The slot's context must have room for
        n * max_keypoints queries.  `keep`: the images' tensors, held until the slot's next enqueue.  While
        set_image_format is on, gray_ptrs are the cameras' raw buffers of that description and (w, h) its size."""
        if self.exchange:
            raise ValueError("frames from device images run on one GPU's whole database")
        self._inputs[slot] = keep
        self._batch[slot] = 1
        self.ctxs[slot].frame_enqueue_images(list(gray_ptrs), w, h, double_size, max_keypoints, Ks, cams, self.params, seed)

    def enqueue_images_batch(self, slot: int, gray_ptrs, n_images: int, w: int, h: int, Ks, cams, seeds,
                             max_keypoints: int = 2048, double_size: bool = True, keep=None):
        """len(seeds) frames of one rig of n_images cameras (frame f's images: gray_ptrs[f n_images : (f + 1) n_images])
        through one FEAT launch per stage and ONE MATCH launch sequence; their objects in result slots 0.. (fetch_batch).
        While set_image_format is on, gray_ptrs are raw buffers of that description, converted by one launch."""
        if self.exchange:
            raise ValueError("frames from device images run on one GPU's whole database")
        B = len(seeds)
        assert 1 <= B * n_images <= capi.MAX_BATCH
        self._inputs[slot] = keep
        self._batch[slot] = B
        self.ctxs[slot].frame_enqueue_images_batch(list(gray_ptrs), n_images, w, h, double_size, max_keypoints, Ks, cams,
                                                   self.params, seeds)

    # ---- Kinect frames: a gray image and a depth map per frame, both on the device ---------------------------
    def enqueue_kinect_batch(self, slot: int, gray_ptrs, depth_ptrs, fill_ptrs, w: int, h: int, seeds, fill_scale=8,
                             bilinear: bool = False, max_keypoints: int = 2048, double_size: bool = True,
                             kind: int = capi.DEPTH_BACKPROJECTION, alpha: float = 0.5, cauchy_scale: float = 0.1, keep=None):
        """len(seeds) frames of moped3d's pipeline (config.hpp:38-49) on the slot's stream: DEPTHFILL of every depth map
        [h, w, 4] in place + its distance map [h, w] (one launch per stage; fill_scale=None: the maps arrive filled, their
        distance maps with them), the maps handed to the frames, FEAT .. FILTER2 of the images as one image batch; objects
        in result slots 0.. (fetch_batch).  The context's depth rules / linkage clusterer are what their setters left.
        While set_image_format is on, gray_ptrs are the camera's raw buffers of that description (bgr8, a Bayer mosaic, ..),
        converted by one launch in front of FEAT; the depth maps are what they were.
        `keep`: the tensors behind the pointers, held until the slot's next enqueue."""
        if self.exchange:
            raise ValueError("frames from device images run on one GPU's whole database")
        B = len(seeds)
        if not (1 <= B <= capi.MAX_BATCH) or len(gray_ptrs) != B or len(depth_ptrs) != B or len(fill_ptrs) != B:
            raise ValueError("one image, one depth map, one distance map and one seed per frame, at most MAX_BATCH frames")
        c = self.ctxs[slot]
        self._inputs[slot] = keep
        self._batch[slot] = B
        if fill_scale is not None:
            c.depth_fill_batch_dev(list(depth_ptrs), list(fill_ptrs), w, h, self.K, fill_scale, bilinear)
        c.frame_set_depth_image_batch(list(depth_ptrs), list(fill_ptrs), w, h, kind, alpha, cauchy_scale)
        c.frame_enqueue_image_batch(list(gray_ptrs), w, h, double_size, max_keypoints, self.K, self.cam, self.params, seeds,
                                    _cam_struct=self._cam)

    def enqueue_kinect_raw_batch(self, slot: int, gray_ptrs, raw_ptrs, raw_fmt: "capi.mh_raw_depth", w: int, h: int, seeds,
                                 fill_scale=8, bilinear: bool = False, max_keypoints: int = 2048, double_size: bool = True,
                                 kind: int = capi.DEPTH_BACKPROJECTION, alpha: float = 0.5, cauchy_scale: float = 0.1,
                                 keep=None):
        """The same from what the sensor delivers (moped3d/moped3d.cpp:279-333): raw_ptrs = one device buffer of raw depth
        per frame, all as raw_fmt (capi.make_raw_depth) describes them.  The [h, w, 4] maps of the batch are built in ONE
        launch into tensors the slot keeps (grown on demand, never shrunk), then everything is enqueue_kinect_batch:
        DEPTHFILL of those maps (fill_scale=None: no DEPTHFILL and no distance maps), the hand-over, the image batch.
        While set_image_format is on, gray_ptrs are the camera's raw buffers too: image and depth as the sensor delivers them.
        -> (maps [B, h, w, 4], distance maps [B, h, w] or None): views of the slot's tensors, valid until its next call."""
        if self.exchange:
            raise ValueError("frames from device images run on one GPU's whole database")
        B = len(seeds)
        if not (1 <= B <= capi.MAX_BATCH) or len(gray_ptrs) != B or len(raw_ptrs) != B:
            raise ValueError("one image, one raw depth buffer and one seed per frame, at most MAX_BATCH frames")
        c = self.ctxs[slot]
        need = B * h * w
        if self._raw_maps[slot] is None or self._raw_maps[slot][0].numel() < need * 4:
            self.streams[slot].synchronize()   # (the slot's stream may still read the tensors this replaces)
            self._raw_maps[slot] = (torch.empty(need * 4, dtype=torch.float32, device=self.dev),
                                    torch.empty(need, dtype=torch.float32, device=self.dev))
        maps = self._raw_maps[slot][0][:need * 4].view(B, h, w, 4)
        dist = self._raw_maps[slot][1][:need].view(B, h, w)
        depth_ptrs = [maps[f].data_ptr() for f in range(B)]
        c.depth_map_from_raw_batch_dev(list(raw_ptrs), raw_fmt, self.K, depth_ptrs, w, h)
        self._inputs[slot] = keep
        self._batch[slot] = B
        fill_ptrs = [dist[f].data_ptr() for f in range(B)] if fill_scale is not None else None
        if fill_scale is not None:
            c.depth_fill_batch_dev(depth_ptrs, fill_ptrs, w, h, self.K, fill_scale, bilinear)
        c.frame_set_depth_image_batch(depth_ptrs, fill_ptrs, w, h, kind, alpha, cauchy_scale)
        c.frame_enqueue_image_batch(list(gray_ptrs), w, h, double_size, max_keypoints, self.K, self.cam, self.params, seeds,
                                    _cam_struct=self._cam)
        return maps, (dist if fill_scale is not None else None)

    def set_depth_fill_mode(self, mode: int):
        """How enqueue_kinect_batch fills the maps, on every slot's context: capi.DEPTH_FILL_REPLAY (the default; maps of
        up to 8192 downscaled pixels, 640 x 480 from fill_scale 8 on) or capi.DEPTH_FILL_LEVELS (the same bytes, maps of
        up to 2^21 downscaled pixels: fill_scale 4, 2 or 1, 1280 x 960 frames)."""
        for c in self.ctxs:
            c.depth_fill_set_mode(mode)

    def set_image_format(self, fmt):
        """What the image pointers of enqueue_images[_batch] and enqueue_kinect[_raw]_batch mean, on every slot's context:
        a capi.make_raw_image description (bgr8, rgb8, bgra8, rgba8, a Bayer mosaic, gray with strides) = the camera's
        buffers, converted to gray on the device by one launch per call (moped3d/moped3d.cpp:249); None = packed 8-bit
        gray, the default.  Not with a sharded database, like every call that takes device images."""
        if fmt is not None and self.exchange:
            raise ValueError("frames from device images run on one GPU's whole database")
        for c in self.ctxs:
            c.frame_set_image_format(fmt)

    def set_linkage_mode(self, mode: int):
        """How the linkage clusterer of the frames runs, on every slot's context: capi.LINKAGE_SCAN (the default; match
        lists of up to 1024 per model) or capi.LINKAGE_ROWMAX (the same clusters, lists of up to 4096)."""
        for c in self.ctxs:
            c.linkage_set_mode(mode)

    def set_filter_depth(self, points_xyz, points_off, f1=None, f2=None, depth_cam=None):
        """FILTER (f1) and / or FILTER2 (f2) of the frames enqueued from now on as moped3d's FILTER_PROJECTION_DEPTH: the
        pose of every object is tested against the frame's depth map, so enqueue_kinect_batch and the other depth-map
        enqueues deliver depth-verified objects.  points_xyz [total, 3], points_off [n_models + 1]: the models' test
        points (the caller's sample); f1, f2: (PlausibleSqDistance, DepthFraction, MinKeypointFraction) or None = that slot
        stays the plain class, both None = off; depth_cam: (K, pose) of the depth map, default the pipeline's camera.
        Such frames run like plain ones: the FILTER steps in the tails of the POSE launches, the frames of
        enqueue_kinect_batch in one launch per stage with every object scored against its own frame's map
        (Context.frame_route() says which way the last frame or batch went); the objects are those of the frames alone.
        Every slot's context is set.  After add_model / replace_model / remove_model the points are stale: call again."""
        if self.exchange:
            raise ValueError("the depth FILTER needs one GPU's whole database: the test points are per global model")
        K, cam = (self.K, self.cam) if depth_cam is None else depth_cam
        for c in self.ctxs:
            if f1 is not None or f2 is not None:
                c.filter_depth_set_points(points_xyz, points_off)
            c.frame_set_filter_depth(f1, f2, K, cam)

    def set_depth_verify(self, params, depth_cam=None):
        """Frames and batches enqueued from now on run moped3d's DEPTH_VERIFY behind FILTER2 (Context.frame_set_depth_verify
        on every slot's context): every object is checked against its own frame's depth map and match lists, the objects
        the reference erases are gone from what fetch() / fetch_batch() / deliver() and the hulls see.  params:
        (FeatureDistance, MaxMultiplier, MaxDistance, DepthFraction) or None = off; depth_cam: (K, pose) of the depth map,
        default the pipeline's camera.  Single-camera frames with a depth map on an unsharded database."""
        if params is not None and self.exchange:
            raise ValueError("DEPTH_VERIFY needs one GPU's whole database: the keypoints are the store's rows per global model")
        K, cam = (self.K, self.cam) if depth_cam is None else depth_cam
        for c in self.ctxs:
            c.frame_set_depth_verify(params, K, cam)

    def verify_records(self, slot: int = 0, frame: int = 0):
        """The DEPTH_VERIFY records of what pipeline slot `slot` (its context) ran last, one per object that left FILTER2
        (capi.VERIFY_DTYPE).  frame: the context's RESULT SLOT index, as fetch_batch's frame_fetch_slot(f) takes it --
        frame f of a batch, 0 for a frame alone (mh_frame_fetch_verify_slot)."""
        return self.ctxs[slot].frame_fetch_verify(frame)

    def set_cluster_wms(self, params: "capi.mh_wms_params | None"):
        """CLUSTER of the frames enqueued from now on as moped3d's CLUSTER_WEIGHTED_MEAN_SHIFT_CPU over the depth map's
        points (Context.frame_set_cluster_wms on every slot's context; None = off).  Single-camera frames with a depth
        map on an unsharded database; a batch runs frame by frame."""
        if params is not None and self.exchange:
            raise capi.MhError("the weighted mean-shift clusterer: single-GPU pipelines only")
        for c in self.ctxs:
            c.frame_set_cluster_wms(params)

    # ---- object hulls: Object::getObjectHull of every object of a frame, computed behind the frame --------------
    def set_hulls(self, max_vertices: int, image: int = 0):
        """Frames and batches enqueued afterwards compute the hulls of their objects (mh_frame_set_hulls; 0 = off, the
        default).  fetch() / fetch_batch() then return (objects, counts, hulls) with hulls = (vertex lists, n_vertices,
        n_behind, bbox_uv) in the order of the objects; deliver() adds the hull block (take_hull_delivery).  Not for a
        sharded database (model indices are shard-local): object_hulls() on the gathered objects instead."""
        if max_vertices and self.exchange:
            raise capi.MhError("hulls behind the frames: single-GPU pipelines only (object_hulls() serves gathered objects)")
        self._hull_vertices = int(max_vertices)
        for c in self.ctxs:
            c.frame_set_hulls(max_vertices, image)

    def object_hulls(self, objects, K, cam, max_vertices: int = 64, slot: int = 0):
        """The hulls of fetched objects (an OBJECT_DTYPE array) in the image (K, cam): mh_object_hulls, a round trip."""
        return self.ctxs[slot].object_hulls(objects["model"], objects["pose"], K, cam, max_vertices)

    def _with_hulls(self, slot, f, res):
        if not getattr(self, "_hull_vertices", 0):
            return res
        objs, counts = res
        return objs, counts, self.ctxs[slot].frame_fetch_hulls(f, max(len(objs), 1), self._hull_vertices)

    def fetch_batch(self, slot: int, B: int):
        return [self._with_hulls(slot, f, self.ctxs[slot].frame_fetch_slot(f)) for f in range(B)]

    # ---- delivery: every batch's objects into pinned host memory, no stream synchronisation ---------------
    def attach_delivery(self, max_objects: int = 16, B: int = capi.MAX_BATCH):
        """One pinned host block per slot for mh_frame_fetch_batch_async / _previous_async: records of
        mh_frame_head + mh_object[max_objects] for up to B frames."""
        self._dlv_cap = max_objects
        self._dlv_dtype = capi.frame_block_dtype(max_objects)
        self._dlv_host = [torch.zeros(capi.frame_block_bytes(B, max_objects), dtype=torch.uint8).pin_memory()
                          for _ in range(self.depth)]
        self._dlv_view = [t.numpy().view(self._dlv_dtype) for t in self._dlv_host]
        self._dlv_pending = [0] * self.depth   # frames of the slot's delivery in flight
        self._dlv_hull_host = None             # (made by the first deliver() with hulls on)

    def deliver(self, slot: int, tag: int = 0, hulls: bool = True):
        """Behind the batch just enqueued in `slot`: its objects (single GPU) or, with a sharded DB, all ranks' objects of
        the slot's PREVIOUS batch (they arrived with this batch's exchange) into the slot's host block."""
        c, B = self.ctxs[slot], self._batch[slot]
        if self.exchange:
            c.frame_fetch_previous_async(self._dlv_cap, self._dlv_host[slot].data_ptr(), tag)
        else:
            c.frame_fetch_batch_async(B, self._dlv_cap, self._dlv_host[slot].data_ptr(), tag)
            hv = getattr(self, "_hull_vertices", 0) if hulls else 0
            if hv:   # the batch's hull records beside its objects, one more stream-ordered copy
                if self._dlv_hull_host is None or self._dlv_hull_dtype != capi.hull_block_dtype(self._dlv_cap, hv):
                    self._dlv_hull_dtype = capi.hull_block_dtype(self._dlv_cap, hv)
                    self._dlv_hull_host = [torch.zeros(capi.MAX_BATCH * self._dlv_hull_dtype.itemsize, dtype=torch.uint8).pin_memory()
                                           for _ in range(self.depth)]
                c.frame_fetch_batch_hulls_async(B, self._dlv_cap, self._dlv_hull_host[slot].data_ptr())
        self._dlv_pending[slot] = B

    def take_delivery(self, slot: int):
        """Waits for the slot's delivery; the B records (a view of the pinned block: copy what must outlive the slot's
        next delivery) or None if nothing was pending."""
        B = self._dlv_pending[slot]
        if not B:
            return None
        self.ctxs[slot].frame_fetch_wait()
        self._dlv_pending[slot] = 0
        return self._dlv_view[slot][:B]

    def take_hull_delivery(self, slot: int, B: int):
        """After take_delivery(slot): the B frames' hull records (capi.hull_block_dtype; a view of the pinned block)."""
        return self._dlv_hull_host[slot].numpy().view(self._dlv_hull_dtype)[:B]

    def previous_objects_batch(self, slot: int):
        """Objects of the B frames of the batch enqueued in `slot` BEFORE the current one, from all ranks."""
        return [self.ctxs[slot].frame_previous_objects(f) for f in range(self._batch[slot])]

    def flush_objects_batch(self, slot: int, B: int):
        """Exchange 2 for the LAST batch of a slot (nothing follows to carry it)."""
        return [self.ctxs[slot].frame_gather_objects(self._comm(slot), f) for f in range(B)]

    def previous_objects(self, slot: int):
        """Objects of the frame enqueued in `slot` BEFORE the current one, from all ranks, as they
        arrived with the current frame's exchange (no collective of its own).  Synchronises the slot."""
        return self.ctxs[slot].frame_previous_objects(0)

    def fetch(self, slot: int):
        """Objects of the frame in `slot` (model ids global), counts[4]; with set_hulls on, their hulls behind them."""
        return self._with_hulls(slot, None, self.ctxs[slot].frame_fetch())

    def gather_objects(self, slot: int):
        """Exchange 2 on its own: every rank's result block -> all ranks; the merged object array
        (rank order = model order)."""
        return self.ctxs[slot].frame_gather_objects(self._comm(slot), 0)

    def synchronize(self):
        for s in self.streams:
            s.synchronize()

    def close(self):
        self.synchronize()
        for m in self.comms:
            m.close()
        self.comms = []
        for c in self.ctxs:
            c.close()
        self.ctxs = []
        if self.lane is not None:
            self.lane.close()
            self.lane = None


def exchange_top2(local: torch.Tensor, world: int, group=None) -> torch.Tensor:
    """Exchange 1: one fused all-gather of every rank's per-query
    local top-2.  local = [3][Q] int32 words (idx1, bits of d1, bits of d2);
    returns [W][3][Q], the block mh_frame_enqueue_rest takes.  The layout of the exchange on
    torch tensors, for the world-size > 1 CPU tests (gloo); on the GPU the same all-gather is
    issued by the library itself (csrc/comm.hip)."""
    import torch.distributed as dist
    Q = local.shape[-1] if local.dim() == 2 else local.numel() // 3
    out = torch.empty(world * 3 * Q, dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, local.contiguous().view(-1), group=group)
    return out.view(world, 3, Q)


def owner_of_model(model: int, n_models: int, world: int, assign: str = "block") -> int:
    """Rank that owns `model` under ShardedDB's partition."""
    if assign == "round-robin":
        return model % world
    for r in range(world):
        if (r * n_models) // world <= model < ((r + 1) * n_models) // world:
            return r
    raise ValueError(model)


class _DevMem:
    """__cuda_array_interface__ view over memory owned by the HIP library."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False),
                                         "version": 2, "strides": None}


def _wrap_int32(ptr, n, dev):
    return torch.as_tensor(_DevMem(ptr, (n,), "<i4"), device=dev)
