"""gpvecchia_amd.build.units(): the one list of the library's objects that every build recipe reads.  Needs no compiler."""
import os
import re

from gpvecchia_amd import build as B


def _objects(plist):
    return [obj for _, obj, _, _ in B.units(plist)]


def _includes(path, seen):
    """the transitive closure of the #include "..." lines of `path`, as absolute paths, into `seen`"""
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M):
        p = os.path.normpath(os.path.join(os.path.dirname(path), inc))
        if p not in seen:
            seen.add(p)
            _includes(p, seen)
    return seen


def test_every_source_is_a_unit():
    sources = {f for f in os.listdir(B.CSRC) if f.endswith((".hip", ".cpp"))}
    assert sources and sources == {src for src, _, _, _ in B.units(B.plist())}


def test_object_names_are_unique():
    objs = _objects(B.plist())
    assert len(objs) == len(set(objs))


def test_dependency_lists_cover_the_includes():
    """What a unit includes, directly or through a header, is in its hand-kept dependency list: a change of any of them
    recompiles it."""
    for src, obj, _, deps in B.units(B.plist()):
        have = {os.path.normpath(os.path.join(B.CSRC, d)) for d in deps}
        need = _includes(os.path.join(B.CSRC, src), set())
        assert all(os.path.exists(p) for p in have | need), (obj, sorted(p for p in have | need if not os.path.exists(p)))
        assert need <= have, (obj, sorted(os.path.relpath(p, B.CSRC) for p in need - have))


def test_per_row_length_rules():
    short = _objects((4, 21))
    assert "sets_p21_lik.o" in short and "sets_p21_lean.o" in short and "sets_p4.o" in short
    assert not [o for o in short if re.search(r"_d\d\.o$", o)] and "sets_p4_lik.o" not in short
    split = _objects((61,))
    assert [o for o in split if o.startswith("sets_")] == ["sets_p61_d3.o", "sets_p61_d2.o", "sets_p61_d1.o", "sets_p61_d0.o",
                                                            "sets_p61.o"]
    flags = {obj: f for _, obj, f, _ in B.units((61,))}
    assert "-DGPV_INST_DISPATCH" in flags["sets_p61.o"] and "-DGPV_INST_DIM=2" in flags["sets_p61_d2.o"]
