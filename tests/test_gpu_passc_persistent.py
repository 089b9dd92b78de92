"""Pass C (csrc/screen_rescore.hip, rescore_kernel) on launches larger than the chip holds wavefronts: (idx1, d1, d2) of the
two-stage path must be the BITS of the exact kernels (mode 0) and of the oracle for every query -- with a device-side
query count, with queries that leave early (all-zero) or are searched by brute force inside pass C among ordinary ones,
at 1 .. 17 and 8191 .. 8193 queries -- and a second launch must find every record slot emptied.

What the suite runs is the product: a wavefront per query in workgroups of four, the kernel's loop run once, no wavefront
walks.  The kernel is written as a loop (wavefront w of a grid of W takes the queries w, w + W, w + 2 W, ...) for the
shapes of the experiment build, which were measured and dropped: two 16-wavefront workgroups per compute
unit whose wavefronts walk, W = 2 x 256 x 16 = 8192 on the MI355X.  The query counts and the places of the degenerate
queries are chosen for THOSE shapes -- 20 011 queries are two full trips and a ragged third, WALK + 5 is the second trip of
the wavefront that took query 5, 8193 is the first count at which a launch walks -- and cover them only when this file
is run by hand on the experiment build:
    make -C moped_amd/csrc EXTRA=-DMH_EXPERIMENTS BUILD=build_exp OUT=../libmoped_hip_exp.so
    MH_LIB_PATH=$PWD/moped_amd/libmoped_hip_exp.so MH_PASSC_WAVES=16 MH_PASSC_K=2 MH_PASSC_PREFETCH=0 \
        python -m pytest -m gpu tests/test_gpu_passc_persistent.py        (MH_PASSC_PREFETCH=1 / 2, MH_PASSC_WAVES=12 likewise)
The DB is small (4 x 2000 rows): what is tested is where a query falls in the launch, not the search."""
import numpy as np
import pytest

import orclib
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu

Q_ALL = 20011
WALK = 8192          # wavefronts of a walking launch of the experiment build (256 compute units); the product does not walk


def _search(c, torch, qn, mode, q_count=None):
    dev = torch.device("cuda:0")
    Q = qn.shape[0]
    tq = torch.from_numpy(np.array(qn, np.float32)).to(dev)     # (a copy: the shared queries are read-only)
    qnorm = torch.from_numpy(orclib.row_norms(qn)).to(dev)
    out = [torch.empty(Q, dtype=t, device=dev) for t in (torch.int32, torch.float32, torch.float32)]
    c.match_set_mode(mode)
    if q_count is None:
        c.match_local_dev(tq.data_ptr(), qnorm.data_ptr(), Q, *[o.data_ptr() for o in out])
    else:     # the count lives on the device, the launches are sized for the capacity Q (the image frames' MATCH)
        n_dev = torch.tensor([q_count], dtype=torch.int32, device=dev)
        c.match_local_counted_dev(tq.data_ptr(), qnorm.data_ptr(), Q, n_dev.data_ptr(), 0, *[o.data_ptr() for o in out])
    c.synchronize()
    c.match_set_mode(-1)
    return [o.cpu().numpy() for o in out]


def _same_bits(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))


def _head(r, n):
    return [x[:n] for x in r]


@pytest.fixture(scope="module")
def env():
    """One context, one DB, 20 011 queries and their exact (mode 0) results, shared and left unchanged."""
    import torch
    c = capi.Context(0)
    db = synth.make_db(4, 2000, seed=3)
    dbn = orclib.normalize(db.desc)
    c.db_upload(dbn, db.model_of, db.xyz, db.n_models)
    base, _, _ = synth.load_sift_fixture()
    qn = orclib.normalize(base[np.random.default_rng(Q_ALL).integers(0, len(base), Q_ALL)])
    exact = _search(c, torch, qn, 0)
    for a in (qn, *exact):
        a.setflags(write=False)
    yield c, torch, dbn, qn, exact
    c.close()


def test_the_walk_wraps_twice_and_ends_ragged(env):
    c, torch, dbn, qn, exact = env
    before = c.match_kernel_launches()["screen"]
    c.match_stats(reset=True)
    two = _search(c, torch, qn, 1)
    assert c.match_kernel_launches()["screen"] == before + 1, "the two-stage path did not run"
    assert _same_bits(two, exact)
    st = c.match_stats()
    assert st["queries"] == Q_ALL and st["brute_force_queries"] == 0


def test_second_launch_finds_every_slot_emptied(env):
    c, torch, dbn, qn, exact = env
    res, cand = [], []
    for _ in range(2):
        c.match_stats(reset=True)
        res.append(_search(c, torch, qn, 1))
        cand.append(c.match_stats()["candidates"])
    assert _same_bits(res[0], exact)
    assert _same_bits(res[1], res[0])
    assert cand[1] == cand[0] > 0


def test_device_side_count_ends_walks_in_the_middle(env):
    c, torch, dbn, qn, exact = env
    n = 17000
    two = _search(c, torch, qn, 1, q_count=n)
    assert (two[0][n:] == -1).all() and np.isposinf(two[1][n:]).all() and np.isposinf(two[2][n:]).all()
    assert _same_bits(_head(two, n), _head(exact, n))
    # (and the launch after it, over all the rows, finds the slots behind the count as empty as the others)
    assert _same_bits(_search(c, torch, qn, 1), exact)


def test_degenerate_queries_in_every_trip_of_the_same_wavefronts(env):
    """All-zero, NaN, x 1e6 and x 1e-6 queries at 5.., 8192 + 5.. and 16384 + 5.. (on a walking shape: the first, second and
    third trip of wavefronts 5 .. 8, each of which meets a different kind in every trip), ordinary queries around them.  The
    all-zero query leaves its iteration early; the NaN and the x 1e6 query are not for f16 to hold and the x 1e-6 one
    has every row inside the margin of every other (its lists overflow): the whole DB on one wavefront, three per trip."""
    c, torch, dbn, qn, exact = env
    q = qn.copy()
    kinds = 4
    for trip in range(3):
        for w in range(kinds):
            i = trip * WALK + 5 + w
            kind = (w + trip) % kinds
            if kind == 0:
                q[i] = 0.0
            elif kind == 1:
                q[i, 0] = np.nan
            elif kind == 2:
                q[i] *= 1e6
            else:
                q[i] *= 1e-6
    c.match_stats(reset=True)
    with np.errstate(all="ignore"):
        two = _search(c, torch, q, 1)
        st = c.match_stats()
        one = _search(c, torch, q, 0)
    assert _same_bits(two, one)
    assert st["brute_force_queries"] == 3 * 3
    plain = np.ones(Q_ALL, bool)
    plain[[t * WALK + 5 + w for t in range(3) for w in range(kinds)]] = False
    assert _same_bits([x[plain] for x in two], [x[plain] for x in exact])


@pytest.mark.parametrize("Q", [1, 15, 16, 17, 8191, 8192, 8193])
def test_workgroup_and_grid_edges(env, Q):
    c, torch, dbn, qn, exact = env
    two = _search(c, torch, qn[:Q], 1)
    if Q <= 17:
        oi, o1, o2 = orclib.match_2nn(dbn, qn[:Q])
        assert _same_bits(two, [oi, o1, o2])
    else:
        assert _same_bits(two, _head(exact, Q))
