"""The park buffer of pass B of the 16x16x32 MATCH launches at its edges (csrc/screen_ab16.hip, screen16_kernel<1, 4>: a
wavefront parks the hits of its sweep in LDS -- mh_screen_park_places of them -- and writes them to their queries' lists at
the end; a hit that finds the buffer full appends from the hit path): one wavefront's sweep leaves exactly as many hits as
the buffer holds, one more, and half as many again, and (idx1, d1, d2) stay bit for bit those of match_kernel /
match_mfma_kernel (mh_match_set_mode 2 / 3) and of the oracle.

How a sweep's hits are counted out: the 128 queries of the wavefront each have two rows at amp 5e-3 in sampled tiles, which
lifts their thresholds above every unstructured row (tests/test_gpu_record_lists.py's docstring: shapes, plan, _near), so
the only hits of the wavefront's sweep over its split are the rows planted here, one record each (different tiles).  A
query's nearest row lies in the split's LAST tile and its second nearest in the tile before: the hits that find the
buffer full are the nearest rows of the last queries, and a record lost on either way loses its query's answer.  (How
many hits took which way is not observable in the product build; the cases are built to the places the library reports.)"""
import numpy as np
import pytest

from moped_amd import capi
from test_gpu_record_lists import SHAPE_4TH, SHAPE_8TH, TILE, _near, _plan, _run_and_check, env  # noqa: F401

pytestmark = pytest.mark.gpu
AMPS = (1e-3, 2e-3, 3e-3)


def _cases():
    park = 240
    return [(SHAPE_8TH, 3, park), (SHAPE_8TH, 3, park + 1), (SHAPE_8TH, 15, 3 * 128), (SHAPE_4TH, 0, 3 * 128)]


@pytest.mark.parametrize("shape,split,n_hits", _cases())
def test_hits_of_one_sweep_around_the_buffer(env, shape, split, n_hits):
    c, torch, rows = env
    park = capi.screen_park_places()
    assert park == 240, "the cases are built around 240 places"
    assert 128 <= n_hits <= len(AMPS) * 128
    Q, N = shape
    sampled, uns, splits = _plan(Q, N)
    assert split < len(splits)
    db, qn = rows(shape)
    rng = np.random.default_rng(21)
    q0 = 2 * 1024 + 5 * 128                      # wavefront 5 of the third 1 024-query workgroup
    j0, j1 = splits[split]
    tiles = [t for t in uns[j0:j1] if t < -(-N // TILE) - 1]
    assert len(tiles) >= len(AMPS)
    want, used = {}, set()
    for i in range(128):
        q = qn[q0 + i]
        for k in range(2):                        # the threshold: two rows in sampled tiles (not the last tile: it may be padded)
            r = sampled[(2 * i + k) % (len(sampled) - 1)] * TILE + i
            assert r not in used
            used.add(r)
            db[r] = _near(rng, q, 5e-3)
        n_i = n_hits // 128 + (1 if i < n_hits % 128 else 0)
        for m in range(n_i):                      # the m-th nearest row in the m-th tile from the split's end
            r = tiles[-1 - m] * TILE + (3 * i) % TILE
            assert r not in used and r < N
            used.add(r)
            db[r] = _near(rng, q, AMPS[m])
            if m == 0:
                want[q0 + i] = r
    two, st, inc = _run_and_check(c, torch, db, qn, planted=range(q0, q0 + 128))
    for qi, r in want.items():
        assert two[0][qi] == r, (qi, int(two[0][qi]), r)
    assert st["brute_force_queries"] == 0, st
