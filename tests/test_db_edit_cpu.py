"""Properties of the numpy splice the GPU tests of mh_db_splice upload as their reference (tests/db_edit_ref.py)."""
import numpy as np
import pytest

import db_edit_ref as ref


def rows(rng, n):
    return rng.random((n, 128), dtype=np.float32), rng.standard_normal((n, 3)).astype(np.float32)


def seeded_db(seed, sizes):
    rng = np.random.default_rng(seed)
    d, x = rows(rng, sum(sizes))
    m = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    return (d, x, m, len(sizes))


SIZES = [(5, 0, 7, 3), (1,), (0, 0), (4, 9, 2, 0), ()]


@pytest.mark.parametrize("sizes", SIZES)
def test_remove_after_insert_is_the_identity(sizes):
    db = seeded_db(1, sizes)
    rng = np.random.default_rng(2)
    for at in range(db[3] + 1):
        for n in (0, 1, 6):
            d, x = rows(rng, n)
            grown = ref.insert(db, at, d, x)
            begin = ref.model_rows(db, at)[0] if at < db[3] else len(db[2])
            assert grown[3] == db[3] + 1 and ref.model_rows(grown, at) == (begin, n)
            assert np.array_equal(grown[0][begin:begin + n], d)
            assert ref.same(ref.remove(grown, at), db)


@pytest.mark.parametrize("sizes", SIZES[:4])
def test_replace_is_remove_then_insert_at_the_same_index(sizes):
    db = seeded_db(3, sizes)
    rng = np.random.default_rng(4)
    for at in range(db[3]):
        for n in (0, 2, 11):
            d, x = rows(rng, n)
            assert ref.same(ref.replace(db, at, d, x), ref.insert(ref.remove(db, at), at, d, x))


def test_model_ids_stay_ascending_and_dense_and_empty_models_survive():
    rng = np.random.default_rng(5)
    db = seeded_db(6, (3, 0, 4, 0, 0, 2))
    sizes = [3, 0, 4, 0, 0, 2]
    for step in range(200):
        op = int(rng.integers(0, 3)) if db[3] else ref.INSERT
        n = int(rng.choice([0, 0, 1, 5]))
        d, x = rows(rng, n)
        if op == ref.INSERT:
            at = int(rng.integers(0, db[3] + 1))
            db = ref.insert(db, at, d, x)
            sizes.insert(at, n)
        elif op == ref.REPLACE:
            at = int(rng.integers(0, db[3]))
            db = ref.replace(db, at, d, x)
            sizes[at] = n
        else:
            at = int(rng.integers(0, db[3]))
            db = ref.remove(db, at)
            del sizes[at]
        assert ref.is_grouped(db) and db[3] == len(sizes) and len(db[2]) == sum(sizes)
        # dense: model i of the table is model i of the rows, empty ones included
        assert [ref.model_rows(db, i)[1] for i in range(db[3])] == sizes
        assert np.array_equal(db[2], np.repeat(np.arange(len(sizes), dtype=np.int32), sizes))
        assert db[0].dtype == np.float32 and db[1].dtype == np.float32 and db[2].dtype == np.int32


def test_rows_outside_the_splice_keep_their_bits_and_their_order():
    db = seeded_db(7, (4, 6, 5))
    d, x = rows(np.random.default_rng(8), 3)
    out = ref.replace(db, 1, d, x)
    assert np.array_equal(out[0][:4], db[0][:4]) and np.array_equal(out[0][7:], db[0][10:])
    assert np.array_equal(out[1][7:], db[1][10:]) and np.array_equal(out[2], [0] * 4 + [1] * 3 + [2] * 5)


def test_out_of_range_models_are_refused():
    db = seeded_db(9, (2, 2))
    for op, at in ((ref.INSERT, 3), (ref.INSERT, -1), (ref.REPLACE, 2), (ref.REMOVE, 2), (ref.REMOVE, -1)):
        with pytest.raises(IndexError):
            ref.splice(db, op, at, *rows(np.random.default_rng(0), 1))
    with pytest.raises(IndexError):
        ref.remove(ref.empty(), 0)
