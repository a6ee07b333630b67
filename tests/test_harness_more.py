"""charon_amd/build.py's MORE_HARNESSES -- the harness rows that came after tests/test_harness_table.py
pinned the names and the build order of HARNESSES -- held to that table's terms: one recipe, named header
lists equal to the compiler's own, a device row's product sources equal to what its source includes, an
id that moves with every hashed file and no other, every source under tests/native/more owned by one
row.  CPU only; nothing here compiles a harness."""
import os
import re
import shutil
import subprocess

import pytest

from charon_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORE = os.path.join(ROOT, "tests", "native", "more")
NAMES = list(build.MORE_HARNESSES)
HOST = [n for n in NAMES if build.MORE_HARNESSES[n].kind == build.HOST]
DEVICE = [n for n in NAMES if build.MORE_HARNESSES[n].kind == build.DEVICE]


def test_the_rows_and_their_place():
    assert "clusterselcheck" in HOST and "clustersumdev" in DEVICE
    assert not set(NAMES) & set(build.HARNESSES)
    stems = [h.stem for h in list(build.HARNESSES.values()) + list(build.MORE_HARNESSES.values())]
    assert len(set(stems)) == len(stems)  # one exported <stem>_build_id each
    for n in NAMES:
        assert build.harness_row(n) is build.MORE_HARNESSES[n]
        assert build.harness_source(n) == os.path.join(MORE, n + (".hip" if n in DEVICE else ".cpp"))
        assert build.harness_path(n) == os.path.join(ROOT, "tests", "native", f"libhbls_{n}.so")
        assert build.harness_build_id(n).startswith(f"hbls-{n}:")
        assert getattr(build, n + "_build_id")() == build.harness_build_id(n)
    for n in build.HARNESSES:  # the table's rows are where they were
        assert os.path.dirname(build.harness_source(n)) == os.path.join(ROOT, "tests", "native")
    seen = []
    real = {n: getattr(build, "build_" + n) for n in NAMES}
    try:
        for n in NAMES:
            setattr(build, "build_" + n, lambda force, verbose, n=n: seen.append(n) if n != NAMES[0] else 1 / 0)
        failed = build.build_more_harnesses(verbose=False)
    finally:
        for n, fn in real.items():
            setattr(build, "build_" + n, fn)
    assert failed == ["build_" + NAMES[0]] and seen == NAMES[1:]  # printed and returned, and the rest is still built


def test_build_runs_them_behind_the_table():
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        src = f.read()
    assert src.index("b.build_test_extras()") < src.index("b.build_more_harnesses()")


@pytest.mark.parametrize("name", [n for n in HOST if build.MORE_HARNESSES[n].headers != build.ALL])
def test_named_headers_are_what_the_source_includes(name):
    r = subprocess.run(["g++", "-std=c++17", "-MM", build.harness_source(name)], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    csrc = os.path.join(ROOT, "charon_amd", "csrc")
    deps = [os.path.normpath(os.path.join(ROOT, d)) for d in r.stdout.replace("\\\n", " ").split()[1:]]
    included = {os.path.basename(d) for d in deps if os.path.dirname(d) == csrc and d.endswith(".h")}
    assert included == set(build.MORE_HARNESSES[name].headers)
    assert len(set(build.MORE_HARNESSES[name].headers)) == len(build.MORE_HARNESSES[name].headers)


@pytest.mark.parametrize("name", DEVICE)
def test_product_sources_are_what_the_device_source_includes(name):
    with open(build.harness_source(name)) as f:
        includes = re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M)
    assert "../devblocks.h" in includes
    assert [os.path.basename(i) for i in includes if i.endswith(".hip")] == list(build.MORE_HARNESSES[name].sources)
    assert all(i == "../../../charon_amd/csrc/" + os.path.basename(i) for i in includes if i.endswith(".hip"))


@pytest.fixture
def tree(tmp_path):
    """A copy of the real sources the ids hash, for a test to append to"""
    root = tmp_path
    shutil.copytree(os.path.join(ROOT, "charon_amd", "csrc"), root / "charon_amd" / "csrc")
    os.makedirs(root / "tests" / "native" / "more")
    for n in NAMES:
        shutil.copy(build.harness_source(n), root / "tests" / "native" / "more")
    shutil.copy(os.path.join(ROOT, "tests", "native", "devblocks.h"), root / "tests" / "native")
    return str(root)


@pytest.mark.parametrize("name", NAMES)
def test_id_moves_with_every_hashed_file_and_no_other(name, tree):
    h = build.MORE_HARNESSES[name]
    assert build.harness_build_id(name, root=tree) == build.harness_build_id(name)
    csrc = sorted(f for f in os.listdir(os.path.join(tree, "charon_amd", "csrc")))
    headers = [f for f in csrc if f.endswith(".h")]
    mine = headers if h.headers == build.ALL else list(h.headers)
    assert set(mine) <= set(headers)
    hashed = [os.path.relpath(build.harness_source(name, tree), tree)] + ["charon_amd/csrc/" + f for f in mine + list(h.sources)] + \
        (["tests/native/devblocks.h"] if h.kind == build.DEVICE else [])

    def touch(rel):
        before = build.harness_build_id(name, root=tree)
        with open(os.path.join(tree, rel), "a") as f:
            f.write("\n// touched\n")
        return before != build.harness_build_id(name, root=tree)
    for rel in hashed:
        assert touch(rel), rel
    unlisted = [f for f in headers if f not in mine]
    assert unlisted or h.headers == build.ALL
    others = ["charon_amd/csrc/" + f for f in unlisted + [f for f in csrc if f.endswith(".hip") and f not in h.sources]] + \
        ([] if h.kind == build.DEVICE else ["tests/native/devblocks.h"])
    for rel in others:
        assert not touch(rel), rel


def test_every_source_of_the_folder_is_owned():
    sources = {f for f in os.listdir(MORE) if f.endswith((".cpp", ".hip"))}
    assert sources == {os.path.basename(build.harness_source(n)) for n in NAMES}
