"""Loading the harnesses of charon_amd/build.py's MORE_HARNESSES on gpu_helpers/harness.py's terms: the
library is the tree's (its embedded id) or the test fails.  Needs no GPU itself."""
import ctypes

from charon_amd import build


def load(name):
    """A row of build.MORE_HARNESSES, built if the tree's is not there, loaded, and held to the tree's
    id through its own <stem>_build_id()."""
    assert name in build.MORE_HARNESSES
    lib = ctypes.CDLL(build.build_harness(name, verbose=False))
    build_id = getattr(lib, build.harness_row(name).stem.lower() + "_build_id")
    build_id.restype = ctypes.c_char_p
    assert build_id().decode() == build.harness_build_id(name)
    return lib
