"""The records of the keyframe store's Python binding: every parameter record against its numpy twin (defaults, twin(), the one coercion every params= argument
goes through), every result record through the one dict helper, and every record's size against the /* N bytes */ include/qn_engine.h states.  Neither a GPU
nor the library is needed: the records are ctypes layouts."""
import ctypes
import importlib
import os
import re
import types
import pytest
from qn_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [("StaticParams", "staticmap", "StaticParams"), ("RangeParams", "freespace", "Params"), ("NormalParams", "mapnormals", "NormalParams"),
          ("OutlierParams", "mapoutliers", "OutlierParams"), ("GroundParams", "mapground", "GroundParams"), ("OccupancyParams", "mapoccupancy", "OccupancyParams"),
          ("DistanceParams", "mapdistance", "DistanceParams"), ("RouteParams", "maproute", "RouteParams"), ("FrontierParams", "mapfrontier", "FrontierParams"),
          ("ViewParams", "mapview", "ViewParams"), ("ClusterParams", "mapclusters", "ClusterParams"), ("LocalizeParams", "maplocalize", "LocalizeParams")]
RESULTS = ["OverlapDir", "Overlap", "FreespaceDir", "Freespace", "OutlierStats", "GroundStats", "GroundGrid", "OccupancyStats", "OccupancyGrid", "OccupancyUpdate",
           "DistanceStats", "RouteStats", "FrontierStats", "FrontierInfo", "ViewInfo", "ViewStats", "ClusterStats", "ClusterInfo", "LocalizeStats"]
INTEGERS = (ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64)


def _open(rec):
    """the fields a caller sees: every field but the reserved and padding ones, in field order"""
    return [(f, t) for f, t in rec._fields_ if not f.startswith(("reserved", "pad"))]


def _pair(name, module, twin):
    return getattr(engine, name), getattr(importlib.import_module("qn_amd." + module), twin)


@pytest.mark.parametrize("name,module,twin", PARAMS)
def test_a_parameter_record_and_its_twin_hold_the_same_defaults(name, module, twin):
    Rec, Twin = _pair(name, module, twin)
    assert all(t is ctypes.c_double or t in INTEGERS for _, t in _open(Rec)), name
    assert bytes(Rec()) == bytes(Rec(**{f: getattr(Twin(), f) for f, _ in _open(Rec)}))
    assert Rec().twin() == Twin() and type(Rec().twin()) is Twin
    assert all(type(getattr(Rec().twin(), f)) is (float if t is ctypes.c_double else int) for f, t in _open(Rec))


@pytest.mark.parametrize("name,module,twin", PARAMS)
def test_every_params_argument_goes_through_one_coercion(name, module, twin):
    Rec, Twin = _pair(name, module, twin)
    r = Rec()
    assert engine._record(Rec, r) is r
    assert type(engine._record(Rec, None)) is Rec and bytes(engine._record(Rec, None)) == bytes(Rec())
    assert type(engine._record(Rec, Twin())) is Rec and bytes(engine._record(Rec, Twin())) == bytes(Rec()) == bytes(Rec.from_twin(Twin()))
    # distinct values, then every integer field as an integer-valued float and every double field as an int: the bytes int(...) and float(...) give
    want = {f: (float(3 + k) if t is ctypes.c_double else 8 + k) for k, (f, t) in enumerate(_open(Rec))}
    loose = types.SimpleNamespace(**{f: (int(v) if isinstance(v, float) else float(v)) for f, v in want.items()})
    got = engine._record(Rec, loose)
    assert type(got) is Rec and bytes(got) == bytes(Rec(**want))
    with pytest.raises(AttributeError):
        engine._record(Rec, (0.3, 0.5))                              # neither the record nor anything with its fields


def _fill(rec, at=1):
    """distinct values in every field, reserved ones included -> the next unused value"""
    for f, t in rec._fields_:
        v = getattr(rec, f)
        if isinstance(v, ctypes.Structure):
            at = _fill(v, at)
        elif isinstance(v, ctypes.Array):
            setattr(rec, f, t(*range(at, at + len(v)))); at += len(v)
        else:
            setattr(rec, f, at); at += 1
    return at


def _expect(rec):
    out = {}
    for f, _ in _open(type(rec)):
        v = getattr(rec, f)
        out[f] = _expect(v) if isinstance(v, ctypes.Structure) else tuple(v) if isinstance(v, ctypes.Array) else v
    return out


@pytest.mark.parametrize("name", RESULTS)
def test_a_result_record_becomes_a_dict_of_its_open_fields(name):
    rec = getattr(engine, name)()
    _fill(rec)
    d = engine._as_dict(rec)
    assert list(d) == [f for f, _ in _open(type(rec))] and not any(k.startswith(("reserved", "pad")) for k in d)
    assert d == _expect(rec)
    for k, v in d.items():
        field = getattr(rec, k)
        if isinstance(field, ctypes.Array):
            assert type(v) is tuple and all(type(x) in (int, float) for x in v) and len(v) == len(field), (name, k)
        elif isinstance(field, ctypes.Structure):
            assert type(v) is dict, (name, k)
        else:
            assert type(v) in (int, float), (name, k)
    if name == "RouteStats":
        assert "reserved0" in dict(rec._fields_) and "reserved" in dict(rec._fields_) and len(d) == len(rec._fields_) - 2


def test_the_stats_twins_take_their_own_fields_by_name():
    for name, module in (("DistanceStats", "mapdistance"), ("RouteStats", "maproute"), ("FrontierStats", "mapfrontier"), ("ViewStats", "mapview")):
        rec = getattr(engine, name)()
        _fill(rec)
        Twin = getattr(importlib.import_module("qn_amd." + module), name)
        assert rec.twin() == Twin(**{f: getattr(rec, f) for f in Twin._fields}) and set(Twin._fields) <= {f for f, _ in _open(type(rec))}, name


def test_every_record_has_the_size_the_header_states():
    h = open(os.path.join(ROOT, "include", "qn_engine.h")).read()
    stated = {c: int(n) for c, n in re.findall(r"\} (qn_\w+);\s*/\* (\d+) bytes \*/", h)}
    seen = 0
    for name in [p[0] for p in PARAMS] + RESULTS:
        Rec = getattr(engine, name)
        c_name = re.match(r"(qn_\w+)", Rec.__doc__).group(1)
        assert ctypes.sizeof(Rec) == stated[c_name], (name, c_name, ctypes.sizeof(Rec), stated[c_name])
        seen += 1
    assert seen == len(PARAMS) + len(RESULTS) == 31
