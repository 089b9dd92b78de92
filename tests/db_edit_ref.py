"""The three edits of the model database as one numpy splice: what mh_db_splice must leave on the device is what
mh_db_upload makes of these arrays (tests/test_gpu_db_edit.py).

A database is (desc [N,128] f32, xyz [N,3] f32, model_of [N] i32, n_models), rows grouped by model in ascending
order; empty models are allowed.  new = old[0, b) ++ rows ++ old[e, N), model ids behind the splice point moved by
+1 (insert), 0 (replace) or -1 (remove) -- Moped::addModel / removeModel, moped2/libmoped/src/moped.cpp:139-159."""
import numpy as np

INSERT, REPLACE, REMOVE = 0, 1, 2   # MH_DB_*


def empty():
    return (np.zeros((0, 128), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.int32), 0)


def model_rows(db, model):
    """(row_begin, n_rows) of `model` (mh_db_model_rows)."""
    _, _, model_of, n_models = db
    assert 0 <= model < n_models
    b = int(np.searchsorted(model_of, model, "left"))
    e = int(np.searchsorted(model_of, model, "right"))
    return b, e - b


def splice(db, op, model, desc=None, xyz=None):
    d, x, m, n_models = db
    if op == INSERT:
        if not 0 <= model <= n_models:
            raise IndexError(model)
        b = e = int(np.searchsorted(m, model, "left"))
        delta = 1
    else:
        if not 0 <= model < n_models:
            raise IndexError(model)
        b, n = model_rows(db, model)
        e = b + n
        delta = 0 if op == REPLACE else -1
    if op == REMOVE:
        desc, xyz = np.zeros((0, 128), np.float32), np.zeros((0, 3), np.float32)
    desc = np.ascontiguousarray(desc, np.float32).reshape(-1, 128)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    assert len(desc) == len(xyz)
    nd = np.concatenate([d[:b], desc, d[e:]])
    nx = np.concatenate([x[:b], xyz, x[e:]])
    nm = np.concatenate([m[:b], np.full(len(desc), model, np.int32), m[e:] + np.int32(delta)]).astype(np.int32)
    return (np.ascontiguousarray(nd), np.ascontiguousarray(nx), nm, n_models + delta)


def insert(db, model, desc, xyz):
    return splice(db, INSERT, model, desc, xyz)


def replace(db, model, desc, xyz):
    return splice(db, REPLACE, model, desc, xyz)


def remove(db, model):
    return splice(db, REMOVE, model)


def is_grouped(db):
    _, _, m, n_models = db
    return bool(np.all(np.diff(m) >= 0)) and (len(m) == 0 or (m[0] >= 0 and m[-1] < n_models))


def same(a, b):
    return (a[3] == b[3] and all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) and p.shape == q.shape
                                 for p, q in zip(a[:3], b[:3])))
