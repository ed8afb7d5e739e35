import os
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import pytest

REPO_ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO_ROOT))


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: tests that must run on the GPU box (full-stack "
        "integration tier; this project has no GPU compute)")


@pytest.fixture()
def tmp_path():
    """Short per-test directory instead of pytest's deeply nested one.

    Backends and the balancer rendezvous on AF_UNIX sockets created
    under the test's directory, and sockaddr_un.sun_path holds at most
    107 bytes: below a long $TMPDIR pytest's
    <tmp>/pytest-of-<user>/pytest-N/<test-name>0/ prefix alone uses
    that up and bind() fails. Keep the prefix to a dozen bytes, and
    fall back to /tmp when $TMPDIR itself is long."""
    base = tempfile.gettempdir()
    if len(base) > 48 and os.access("/tmp", os.W_OK | os.X_OK):
        base = "/tmp"
    d = tempfile.mkdtemp(prefix="bt-", dir=base)
    yield Path(d)
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="session", autouse=True)
def built_native():
    """Build the native tree once per test session if it is stale."""
    subprocess.run(["make", "-j8"], cwd=REPO_ROOT, check=True,
                   capture_output=True)
    yield
