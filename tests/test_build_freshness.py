"""Build robustness (CPU): what makes the library stale, and what must not.

* make's view: every header an object includes is a prerequisite of it -- editing ntt_wide.hip.h or the generated wide_asm.inc
  re-compiles every host object that includes it (the round-2 Makefile left a stale library behind), editing the LDS transform
  kernels re-compiles the lds_inst objects and leaves the host objects alone, editing a header one subsystem owns re-compiles
  that subsystem's object only.
* build.py's view: freshness is a content hash in lib/.build_stamp, so a copy of the tree with every mtime reset (the GPU box's
  snapshot) does not rebuild, and a one-byte edit does."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "gpu-homomorphic-encryption_amd")
CSRC = os.path.join(PKG_DIR, "csrc")


def _make_plan(touched):
    """Objects `make -n` would rebuild if `touched` (a file in csrc/) were newer than everything (-W = pretend it was just modified)."""
    res = subprocess.run(["make", "-C", CSRC, "-n", "-W", touched], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return sorted({tok.split("/")[-1] for line in res.stdout.splitlines() if " -o " in line for tok in [line.split(" -o ", 1)[1].split()[0]]})


@pytest.fixture(scope="module")
def built(pkg):
    pkg.build_library()
    return importlib.import_module(pkg.__name__ + ".build")


HOST_OBJECTS = {"core.o", "literal.o", "sampling.o", "engine.o", "transforms.o", "keyswitch.o", "rns.o"}


def _includers(header):
    """Host objects whose source includes `header`, directly or through another header: read from the sources, not from make."""
    def closure(path, seen):
        with open(os.path.join(CSRC, path)) as f:
            for inc in re.findall(r'^#include "([^"/]+)"', f.read(), re.M):
                if inc not in seen:
                    seen.add(inc)
                    closure(inc, seen)
        return seen
    return {o for o in HOST_OBJECTS if header in closure(o[:-2] + ".hip", set())}


@pytest.mark.parametrize("header", ["wide_asm.inc", "ntt_wide.hip.h", "ntt_word.hip.h", "ntt256.hip.h", "ntt_field.hip.h"])
def test_editing_a_header_of_the_host_unit_rebuilds_it(built, header):
    plan = _make_plan(header)
    users = _includers(header)
    assert users and users <= set(plan) and "libfhe_hip.so" in plan, plan
    assert HOST_OBJECTS & set(plan) == users, plan


def test_editing_the_lds_kernels_rebuilds_every_instance_but_not_the_host_unit(built):
    plan = _make_plan("ntt_lds.hip.h")
    assert not HOST_OBJECTS & set(plan) and "libfhe_hip.so" in plan
    assert sum(1 for o in plan if o.startswith("lds_F")) == 17, plan
    assert HOST_OBJECTS <= set(_make_plan("ntt_field.hip.h")) and "lds_F32_13.o" in _make_plan("ntt_field.hip.h")


def test_editing_a_header_one_subsystem_owns_rebuilds_that_object_only(built):
    for header, owner in [("galois.hip.h", "keyswitch.o"), ("sampling.hip.h", "sampling.o"), ("ntt256_rns.hip.h", "rns.o"),
                          ("ntt256_literal.hip.h", "literal.o"), ("ntt256_keyswitch.hip.h", "keyswitch.o"), ("ntt256_transforms.hip.h", "transforms.o")]:
        plan = _make_plan(header)
        assert HOST_OBJECTS & set(plan) == {owner} and "libfhe_hip.so" in plan, (header, plan)
        assert not any(o.startswith("lds_") for o in plan), (header, plan)


def test_up_to_date_tree_has_nothing_to_do(built):
    res = subprocess.run(["make", "-C", CSRC, "-n"], capture_output=True, text=True)
    assert res.returncode == 0 and " -o " not in res.stdout, res.stdout[-2000:]
    assert built.is_fresh()
    built.build_library()
    assert built.last_build == {"compiled": [], "seconds": 0.0, "skipped": True}


def test_snapshot_with_reset_mtimes_is_fresh_and_an_edit_is_not(built, tmp_path):
    """Copy the package (sources + lib/) WITHOUT preserving mtimes, then set every mtime to one instant, as a snapshot tool may:
    the stamp still matches, so build_library() returns without calling make.  Appending a byte to wide_asm.inc flips it."""
    import importlib.util
    dst = tmp_path / "gpu-homomorphic-encryption_amd"
    shutil.copytree(PKG_DIR, dst, ignore=shutil.ignore_patterns("obj", "__pycache__", ".pytest_cache"), copy_function=shutil.copyfile)
    os.makedirs(tmp_path / "include"); shutil.copyfile(os.path.join(ROOT, "include", "fhe_hip.h"), tmp_path / "include" / "fhe_hip.h")
    for d, _, files in os.walk(tmp_path):
        for f in files:
            os.utime(os.path.join(d, f), (1_000_000_000, 1_000_000_000))
    spec = importlib.util.spec_from_file_location("build_copy", dst / "build.py")
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    assert b.source_hash() == built.source_hash()
    assert b.is_fresh()
    assert b.build_library() == str(dst / "lib" / "libfhe_hip.so") and b.last_build["skipped"] is True
    with open(dst / "csrc" / "wide_asm.inc", "a") as f:
        f.write("\n")
    assert not b.is_fresh()
