"""The device buffer pools the seven context-free pan entries keep between calls (pga_host_pan.hpp): one child process under a timeout
of its own calls every entry, releases the pools and calls them again at growing and shrinking shapes (tests/support/pool_direct.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT = os.path.join(ROOT, "tests", "support", "pool_direct.py")

pytestmark = pytest.mark.gpu


def test_release_reaches_every_pool(built):
    r = subprocess.run([sys.executable, DIRECT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, cwd=ROOT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]
