"""Loading the test harnesses of charon_amd/build.py: every fixture gets its library from here, so
each one is the tree's (its embedded id) or the test fails.  Needs no GPU itself."""
import ctypes
import os

import pytest

from charon_amd import build


def load(name):
    """A single-file harness of build.HARNESSES, built if the tree's is not there, loaded, and held
    to the tree's id through its own <stem>_build_id()."""
    lib = ctypes.CDLL(build.build_harness(name, verbose=False))
    build_id = getattr(lib, build.HARNESSES[name].stem.lower() + "_build_id")
    build_id.restype = ctypes.c_char_p
    assert build_id().decode() == build.harness_build_id(name)
    return lib


def load_devblocks(which):
    """A device block harness ("64", "128" or one of build.DEVBLOCKS_OWN), loaded only if it was built
    from this tree (its embedded id); otherwise built now (the two block builds together), and a
    failure of that fails the test with the id in the message."""
    path, want = build.devblocks_path(which), build.devblocks_build_id(which)
    if not os.path.exists(path) or build.embedded_devblocks_id(path) != want:
        try:
            build.build_devblocks(verbose=False, builds=[which] if which in build.DEVBLOCKS_OWN else None)
        except Exception as e:  # noqa: BLE001
            pytest.fail(f"the {which} harness is not the tree's ({want}) and does not build: {e}")
    lib = ctypes.CDLL(path)
    lib.db_build_id.restype = ctypes.c_char_p
    assert lib.db_build_id().decode() == want
    return lib
