"""The checksum path of the asynchronous learner-state save on the device (dqnhip_state_crc32_device: k_state_crc's one thread per
1 KB chunk with slice-by-4 tables in LDS, then the GF(2) fold of the chunks) against Python's zlib.crc32.  Integers only: every
comparison is equality.  Lengths sit around the 16-byte load, the chunk and several chunks; `misalign` moves the buffer's first
byte off the 16-byte boundary, so chunks start inside a 16-byte unit and the single-byte head and tail loops run."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 1024                    # kCrcChunk (dqn-hfo_amd/csrc/state_image.h)
LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, (1 << 20) + 13]
_RNG = np.random.default_rng(77)
_RANDOM = _RNG.integers(0, 256, max(LENGTHS), dtype=np.uint8).tobytes()
_WANT = {n: zlib.crc32(_RANDOM[:n]) for n in LENGTHS}


@pytest.fixture(scope="module")
def dqn(pkg, gpu):
    d = pkg.DQN(58, minibatch=32, hidden=(64, 128), memory=96, seed=3)
    yield d
    d.close()


@pytest.mark.parametrize("misalign", [0, 1, 2, 3, 4, 8, 15])
def test_device_crc_equals_zlib(dqn, misalign):
    for n in LENGTHS:
        got = dqn.state_crc32_device(_RANDOM[:n], misalign)
        assert got == _WANT[n], (n, misalign, hex(got), hex(_WANT[n]))
    for fill in (b"\x00", b"\xff"):
        for n in (1, 65, CHUNK + 1, 2 * CHUNK + 7):
            assert dqn.state_crc32_device(fill * n, misalign) == zlib.crc32(fill * n), (fill, n, misalign)


def test_misalign_outside_0_15_is_refused(pkg, dqn):
    for bad in (-1, 16, 64):
        with pytest.raises(pkg.DQNFatal, match="dqnhip_state_crc32_device: misalign %d is outside 0" % bad):
            dqn.state_crc32_device(b"abc", bad)
    assert dqn.state_crc32_device(b"abc", 15) == zlib.crc32(b"abc")
