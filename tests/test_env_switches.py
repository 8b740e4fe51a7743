"""The environment does not pick kernels: the only FQSS_* variables the package reads are process-level settings (they cross into child
processes or belong to the test harness); the library reads one, the selector of a test's reference kernel; every other flag is a
module constant that tests patch."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fqss_amd")

PYTHON_ENV = {"FQSS_LIB", "FQSS_DEBUG_CARRIER", "FQSS_DETERMINISTIC", "FQSS_DIST_BACKEND", "FQSS_FORCE_DIST", "FQSS_FORCE_BUCKETS",
              "FQSS_DIST_TIMEOUT_S", "FQSS_NPROC", "FQSS_GROUP_WGRAD"}
C_ENV = {"FQSS_GNQ_APPLY_V1"}


def _files(*patterns):
    return sorted(f for p in patterns for f in glob.glob(os.path.join(PKG, p), recursive=True))


def _env_names(files):
    names = set()
    for f in files:
        with open(f, errors="replace") as fh:
            for line in fh:
                if "environ" in line or "getenv" in line:
                    names.update(re.findall(r"FQSS_[A-Z0-9_]+", line))
    return names


def test_environment_reads_are_the_documented_ones():
    py = _files("**/*.py")
    assert len(py) > 20
    assert _env_names(py) == PYTHON_ENV
    assert _env_names(_files("csrc/**/*.hip", "csrc/**/*.h", "csrc/**/*.cpp")) == C_ENV
    with open(os.path.join(ROOT, "README.md")) as fh:
        readme = fh.read()
    missing = sorted(n for n in PYTHON_ENV | C_ENV if not re.search(n + r"\b", readme))
    assert not missing, missing
    needle = '__import__("os")'
    inline = []
    for dirpath, _, names in os.walk(PKG):
        for n in names:
            with open(os.path.join(dirpath, n), "rb") as fh:
                if needle.encode() in fh.read():
                    inline.append(os.path.join(dirpath, n))
    assert not inline, inline
