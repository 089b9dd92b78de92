"""Model sets from rows and back to `.moped.xml` (mh_models_add_rows, mh_models_write_xml): host code, no GPU.

The text is compared character for character with tests/planar_ref.py (sXML::print + toString of the tree
Moped::createPlanarModelsFromImages builds, moped2/libmoped/src/moped.cpp:211-233); what the project's reader -- pinned to
the reference's sXML.hpp elsewhere -- and, where built, the reference's own parse make of the file is compared on bits."""
import ctypes as C
import os

import numpy as np
import pytest

import orclib
import planar_ref as ref
from moped_amd import capi


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(0x9E0)
    n = 37
    desc = np.abs(rng.normal(size=(n, 128))).astype(np.float32)
    desc /= np.linalg.norm(desc, axis=1, keepdims=True)
    xyz = rng.uniform(-0.4, 0.4, (n, 3)).astype(np.float32)
    # values that exercise %g: zero, a small power of ten, more than 6 digits, minus zero, a denormal, big and tiny exponents
    special = np.array([0.0, 1e-05, 123456.7, -0.0, 1e-42, 1e+20, 9.999995e-5, 0.1, 1234567.0, -2.5e-7], np.float32)
    desc[0, :len(special)] = special
    xyz[0] = [0.0, 1e-05, 123456.7]
    xyz[1] = [-0.0, 1e-42, -1e+10]
    xyz[:, 2][2:] = 0.0   # form 0's z
    desc.setflags(write=False)
    xyz.setflags(write=False)
    return desc, xyz


def test_write_xml_is_the_reference_text_and_reads_back(rows, tmp_path):
    desc, xyz = rows
    s = capi.ModelSet()
    s.add_rows("taught model", desc, xyz)
    assert s.n_models == 1 and s.n_rows == len(desc) and s.name(0) == "taught model"
    assert np.array_equal(bits(s.desc), bits(desc)) and np.array_equal(bits(s.xyz), bits(xyz))   # kept as given
    assert np.array_equal(bits(s.model_range(0)[2]), bits(ref.bbox(xyz)))
    path = str(tmp_path / "taught.moped.xml")
    s.write_xml(0, path)
    text = open(path, "rb").read().decode("latin-1")
    assert text == ref.xml_text("taught model", desc, xyz)
    assert ' p3d="0 1e-05 123457"/>' in text and ' p3d="-0 1.00053e-42 -1e+10"/>' in text
    # toString's cases one by one, as the library printed them: row 0's first descriptor values
    first = text.split('desc="', 1)[1].split('"', 1)[0].split(" ")
    assert first[:10] == ["0", "1e-05", "123457", "-0", "1.00053e-42", "1e+20", "9.99999e-05", "0.1", "1.23457e+06", "-2.5e-07"]
    assert first[:10] == [ref.g(v) for v in desc[0, :10]]
    # the project's own reader: the rows rounded to 6 significant digits, the same name, the box of those rows
    back = capi.ModelSet()
    back.add_xml(path)
    want_d, want_x = ref.round6(desc), ref.round6(xyz)
    assert back.n_models == 1 and back.name(0) == "taught model" and back.n_rows == len(desc)
    assert np.array_equal(bits(back.desc), bits(want_d)) and np.array_equal(bits(back.xyz), bits(want_x))
    assert np.array_equal(back.model_range(0)[2], ref.bbox(want_x))
    # ... and the Python restatement of sXML's tokenizer agrees
    py = orclib.parse_model_xml(path)
    assert py["name"] == "taught model" and np.array_equal(bits(py["desc"]), bits(want_d))
    assert np.array_equal(bits(py["xyz"]), bits(want_x))


@pytest.mark.skipif(not orclib.ref_available(), reason="reference libraries not built (oracle/_ref)")
def test_reference_parse_reads_the_written_file(rows, tmp_path):
    desc, xyz = rows
    s = capi.ModelSet()
    s.add_rows("taught", desc, xyz)
    path = str(tmp_path / "taught.moped.xml")
    s.write_xml(0, path)
    got = orclib.ref_model_xml(path)
    assert got is not None and got["name"] == "taught" and got["n_bad_len"] == 0
    assert np.array_equal(bits(got["desc"]), bits(ref.round6(desc)))
    assert np.array_equal(bits(got["xyz"]), bits(ref.round6(xyz)))
    assert np.array_equal(got["bbox"], ref.bbox(ref.round6(xyz)))


def test_empty_model_is_a_childless_points_element(tmp_path):
    s = capi.ModelSet()
    s.add_rows("nothing", np.zeros((0, 128), np.float32), np.zeros((0, 3), np.float32))
    path = str(tmp_path / "nothing.moped.xml")
    s.write_xml(0, path)
    assert open(path).read() == ref.xml_text("nothing", np.zeros((0, 128)), np.zeros((0, 3))) == \
        '<Model name="nothing">\n\t<Points/>\n</Model>\n'
    assert np.array_equal(s.model_range(0)[2], ref.bbox(np.zeros((0, 3))))
    back = capi.ModelSet()
    back.add_xml(path)
    assert back.n_models == 1 and back.n_rows == 0 and back.name(0) == "nothing"


def test_add_rows_replaces_by_name_and_survives_save_load(rows, tmp_path):
    desc, xyz = rows
    s = capi.ModelSet()
    s.add_rows("a", desc[:10], xyz[:10])
    s.add_rows("b", desc[10:30], xyz[10:30])
    s.add_rows("c", desc[30:], xyz[30:])
    s.add_rows("b", desc[:5], xyz[:5])   # a known name replaces that model and keeps its place (moped.cpp:141-146)
    assert [s.name(i) for i in range(s.n_models)] == ["a", "b", "c"]
    assert [s.model_range(i)[:2] for i in range(3)] == [(0, 10), (10, 5), (15, len(desc) - 30)]
    want_d = np.concatenate([desc[:10], desc[:5], desc[30:]])
    want_x = np.concatenate([xyz[:10], xyz[:5], xyz[30:]])
    assert np.array_equal(bits(s.desc), bits(want_d)) and np.array_equal(bits(s.xyz), bits(want_x))
    assert np.array_equal(s.model_of, np.repeat(np.arange(3, dtype=np.int32), [10, 5, len(desc) - 30]))
    assert np.array_equal(bits(s.model_range(1)[2]), bits(ref.bbox(xyz[:5])))
    path = str(tmp_path / "set.mopeddb")
    s.save(path)
    m = capi.ModelSet.load(path)
    assert [m.name(i) for i in range(m.n_models)] == ["a", "b", "c"]
    assert np.array_equal(bits(m.desc), bits(want_d)) and np.array_equal(bits(m.xyz), bits(want_x))
    for i in range(3):
        assert m.model_range(i)[:2] == s.model_range(i)[:2]
        assert np.array_equal(bits(m.model_range(i)[2]), bits(s.model_range(i)[2]))
    # a mapped set is read-only
    with pytest.raises(capi.MhError):
        m.add_rows("d", desc[:1], xyz[:1])
    # rows that are views of the set's own arrays
    s.add_rows("a", s.desc[10:15], s.xyz[10:15])
    assert np.array_equal(bits(s.desc[:5]), bits(desc[:5])) and s.model_range(0)[:2] == (0, 5)


def test_add_rows_and_write_xml_reject_bad_arguments(rows, tmp_path):
    desc, xyz = rows
    s = capi.ModelSet()
    L = s.L
    d, x = np.ascontiguousarray(desc), np.ascontiguousarray(xyz)
    assert L.mh_models_add_rows(s.h, b"m", capi._ptr(d), capi._ptr(x), -1) == -1
    assert L.mh_models_add_rows(s.h, b"m", None, capi._ptr(x), 3) == -1
    assert L.mh_models_add_rows(s.h, b"m", capi._ptr(d), None, 3) == -1
    assert L.mh_models_add_rows(s.h, None, capi._ptr(d), capi._ptr(x), 3) == -1
    assert L.mh_models_add_rows(None, b"m", capi._ptr(d), capi._ptr(x), 3) == -1
    assert s.n_models == 0 and s.n_rows == 0
    assert L.mh_models_add_rows(s.h, b"m", None, None, 0) == 0 and s.n_models == 1   # no rows: no arrays needed
    path = str(tmp_path / "x.xml").encode()
    assert L.mh_models_write_xml(s.h, 1, path) == -1 and L.mh_models_write_xml(s.h, -1, path) == -1
    assert L.mh_models_write_xml(s.h, 0, None) == -1 and L.mh_models_write_xml(None, 0, path) == -1
    assert L.mh_models_write_xml(s.h, 0, str(tmp_path / "no" / "such" / "dir.xml").encode()) == -1
    assert not os.path.exists(path)
