"""niidmix.build rebuilds the library when any file it is compiled from changed: the root source
csrc/niidmix.hip, a csrc/*.inc it includes, or include/niidmix.h (no compiler run, no GPU)."""
import os
import re

import pytest

from conftest import PKG_ROOT


@pytest.fixture
def tree(tmp_path, monkeypatch):
    """A library newer than a root source, two .inc files and a header, all under tmp_path."""
    from niidmix import build
    csrc = tmp_path / "csrc"
    csrc.mkdir()
    files = {"root": csrc / "niidmix.hip", "inc": csrc / "model_gnlenet.inc", "inc2": csrc / "other.inc",
             "header": tmp_path / "niidmix.h", "lib": tmp_path / "libniidmix.so"}
    for i, k in enumerate(("root", "inc", "inc2", "header", "lib")):
        files[k].write_text(k)
        os.utime(files[k], (1000 + i, 1000 + i))
    monkeypatch.setattr(build, "LIB", str(files["lib"]))
    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "SOURCES", [str(files["root"])])
    monkeypatch.setattr(build, "HEADERS", [str(files["header"])])
    return build, files


def test_fresh_library_needs_no_build(tree):
    build, files = tree
    assert sorted(build.dependencies()) == sorted(str(files[k]) for k in ("root", "inc", "inc2", "header"))
    assert not build.needs_build()


@pytest.mark.parametrize("which", ["root", "inc", "inc2", "header"])
def test_touched_dependency_needs_build(tree, which):
    build, files = tree
    os.utime(files[which], (2000, 2000))
    assert build.needs_build()


def test_missing_library_needs_build(tree):
    build, files = tree
    files["lib"].unlink()
    assert build.needs_build()


def test_every_included_inc_is_a_dependency():
    from niidmix import build
    csrc = os.path.join(PKG_ROOT, "csrc")
    root = os.path.join(csrc, "niidmix.hip")
    assert build.SOURCES == [root]
    included = re.findall(r'^\s*#include "([^"/]+)"', open(root).read(), re.M)
    assert included, "the root source includes family files from csrc/"
    deps = build.dependencies()
    for name in included:
        path = os.path.join(csrc, name)
        assert os.path.isfile(path), name
        assert path in deps, name
    assert root in deps and os.path.join(build.REPO, "include", "niidmix.h") in deps
