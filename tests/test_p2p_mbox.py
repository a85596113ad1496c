"""The per-pair mailbox of tl/cdna4's device active-set bcast
(src/tl/cdna4/p2p_mbox.h), driven by three host processes with no GPU:
build/test_p2p_mbox (tests/native/test_p2p_mbox.cc)."""

import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_p2p_mbox_native():
    """Ring wrap-around past the depth, ring-full back-pressure, per-pair
    independence, error-status ack, attach-before-create."""
    binary = os.path.join(REPO, "build", "test_p2p_mbox")
    assert os.path.exists(binary), "build/test_p2p_mbox not built (make)"
    p = subprocess.run([binary], capture_output=True, text=True,
                       timeout=120)
    sys.stdout.write(p.stdout[-500:])
    sys.stderr.write(p.stderr[-2000:])
    assert p.returncode == 0
    assert "P2P_MBOX_OK" in p.stdout
