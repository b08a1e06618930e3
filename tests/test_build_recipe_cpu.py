"""The one build recipe of libunerf (lib.compile_command / lib._source_digest), without compiling anything.

The digest decides whether csrc/libunerf.so is rebuilt: it has to move with every text a build reads, listed anywhere or
not.  The command line is what the product build and every A/B variant (benchmarks/build_variant.py) run: every source,
every flag, and a replacement only in the place of the source it replaces."""
import importlib.util
import os
import shutil

import pytest

from uncertainty_nerf_gs_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTS = sorted(n for n in os.listdir(lib.CSRC) if n.endswith((".hip", ".hpp", ".inc")))


@pytest.fixture()
def csrc_copy(tmp_path):
    dst = tmp_path / "csrc"
    dst.mkdir()
    for n in TEXTS:
        shutil.copy(os.path.join(lib.CSRC, n), dst / n)
    return dst


def test_digest_of_a_copy_is_the_digest_of_csrc(csrc_copy):
    assert set(lib.SOURCES) <= set(TEXTS) and len(TEXTS) > len(lib.SOURCES)      # the sources and the texts they include
    assert lib._source_digest(str(csrc_copy)) == lib._source_digest()


def test_digest_moves_with_a_new_header(csrc_copy):
    before = lib._source_digest(str(csrc_copy))
    (csrc_copy / "unerf_new_header.hpp").write_text("// a header nobody listed\n")
    assert lib._source_digest(str(csrc_copy)) != before


@pytest.mark.parametrize("name", TEXTS)
def test_digest_moves_with_every_text(csrc_copy, name):
    before = lib._source_digest(str(csrc_copy))
    with open(csrc_copy / name, "a") as f:
        f.write("// edited\n")
    assert lib._source_digest(str(csrc_copy)) != before


def build_variant():
    spec = importlib.util.spec_from_file_location("build_variant", os.path.join(ROOT, "benchmarks", "build_variant.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_variant_command_holds_every_source_and_flag():
    out, extra, replace = build_variant().variant("x", None, ["-DUNERF_SOMETHING=1"])
    assert replace is None and out.endswith(os.path.join("benchmarks", "build_probe", "libunerf_x.so"))
    cmd = lib.compile_command(out, extra, replace)
    for s in lib.SOURCES:
        assert os.path.join(lib.CSRC, s) in cmd
    for f in lib.HIPCC_FLAGS:
        assert f in cmd
    assert cmd[cmd.index("-o") + 1] == out
    assert cmd.count("-DUNERF_SOMETHING=1") == 1
    assert [c for c in cmd if c != "-DUNERF_SOMETHING=1"] == lib.compile_command(out)      # the product's line otherwise


def test_nerf_source_replaces_one_source_and_removes_nothing_else(tmp_path):
    copy = str(tmp_path / "unerf_nerf_patched.hip")
    out, extra, replace = build_variant().variant("y", copy, [])
    cmd, plain = lib.compile_command(out, extra, replace), lib.compile_command(out)
    nerf = os.path.join(lib.CSRC, "unerf_nerf.hip")

    def sources(c):
        return c[c.index(out) + 1:]

    assert nerf in sources(plain)
    assert sources(cmd) == [copy if p == nerf else p for p in sources(plain)]              # in its place, nothing else gone
    for f in lib.HIPCC_FLAGS:
        assert f in cmd
    assert all(c in cmd for c in plain if c != nerf)
    with pytest.raises(lib.UnerfError):
        lib.compile_command(out, (), ("unerf_missing.hip", copy))
