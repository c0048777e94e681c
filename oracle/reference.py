"""The real reference library, for the tests that link against it (tests/test_integration_shim.py).

Nothing of SoundSwallower is kept in this repository.  When a SoundSwallower source tree is found
at build time, build() configures and builds its static library out of tree into oracle/_ref/
(kept out of git) and copies its public headers beside it:

    oracle/_ref/include/   the reference's include/ (soundswallower/*.h)
    oracle/_ref/build/     the CMake build: config.h, libsoundswallower.a

The source tree is $SSW_REFERENCE_DIR, else the first of DEFAULT_TREES that holds the public
headers: a `reference` checkout beside this repository, the home directory's, or /root/reference
(the tree the oracle's file:line citations refer to).  Without one nothing is built, and the tests
that need it say so.
"""
from __future__ import annotations

import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(_HERE, "_ref")
INCLUDE = os.path.join(REF, "include")
BUILD = os.path.join(REF, "build")
LIBRARY = os.path.join(BUILD, "libsoundswallower.a")


DEFAULT_TREES = (os.path.join(os.path.dirname(os.path.dirname(_HERE)), "reference"),
                 os.path.join(os.path.expanduser("~"), "reference"),
                 "/root/reference")


def source_tree():
    """The SoundSwallower source tree to take the headers from (and to build, when it holds the
    sources too), or None."""
    env = os.environ.get("SSW_REFERENCE_DIR")
    for c in [env] if env else DEFAULT_TREES:
        if os.path.isdir(os.path.join(c, "include", "soundswallower")):
            return os.path.abspath(c)
    return None


def have_headers() -> bool:
    return os.path.isdir(os.path.join(INCLUDE, "soundswallower"))


def available() -> bool:
    """build() has made the headers and the library."""
    return (have_headers() and os.path.isfile(os.path.join(BUILD, "config.h"))
            and os.path.isfile(LIBRARY))


def build():
    """Copy the reference's headers and build its library into oracle/_ref/ (the library only
    where the tree holds the sources and cmake is installed); returns the source tree, or None
    when there is none (an earlier oracle/_ref/ is then left as it is)."""
    src = source_tree()
    if src is None:
        return None
    # contents only: the source tree may be read-only, and its modes would stop the next rebuild
    shutil.rmtree(INCLUDE, ignore_errors=True)
    top = os.path.join(src, "include")
    for d, _, files in os.walk(top):
        dst = os.path.join(INCLUDE, os.path.relpath(d, top))
        os.makedirs(dst, exist_ok=True)
        for f in files:
            shutil.copyfile(os.path.join(d, f), os.path.join(dst, f))
    if (shutil.which("cmake") is None or not os.path.isdir(os.path.join(src, "src"))
            or not os.path.isfile(os.path.join(src, "CMakeLists.txt"))):
        return src
    cache = os.path.join(BUILD, "CMakeCache.txt")
    if os.path.exists(cache):             # configured from another source tree: start afresh
        with open(cache, errors="replace") as fh:
            if f"CMAKE_HOME_DIRECTORY:INTERNAL={src}\n" not in fh.read():
                shutil.rmtree(BUILD)
    os.makedirs(BUILD, exist_ok=True)
    for cmd in (["cmake", "-S", src, "-B", BUILD, "-DCMAKE_BUILD_TYPE=Release",
                 "-DBUILD_TESTING=OFF"],
                ["cmake", "--build", BUILD, "--target", "soundswallower", "-j", "8"]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("reference build failed: " + " ".join(cmd) + "\n"
                               + r.stdout[-2000:] + r.stderr[-2000:])
    return src
