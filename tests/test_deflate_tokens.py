"""tests/deflate_tokens.py pinned against zlib and against deflate_writer.py: the tokens it reads from zlib's own streams
(levels 1 / 6 / 9, default / fixed / RLE strategies) and from the hand-built spec corpus must stand for the input, and it
must use exactly the stream's bytes.  No GPU."""
import zlib

import numpy as np
import pytest

from tests import deflate_tokens, deflate_writer
from tests.test_inflate import kinds


@pytest.mark.parametrize("strategy", [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE])
@pytest.mark.parametrize("level", [1, 6, 9])
def test_tokens_of_zlib_streams_stand_for_the_input(level, strategy):
    rng = np.random.default_rng(level)
    seen = set()
    for size in (0, 1, 2, 3, 300, 20000):
        for name, data in kinds(rng, size):
            c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
            stream = c.compress(data[:size // 2]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[size // 2:]) + c.flush()
            blocks, used = deflate_tokens.read(stream)
            assert used == len(stream) and blocks[-1]["final"] and not any(b["final"] for b in blocks[:-1])
            assert deflate_tokens.replay(blocks) == data, (name, size)
            for b in blocks:
                seen.add(b["btype"])
                for t in b["tokens"]:
                    assert isinstance(t, int) or (3 <= t[0] <= 258 and 1 <= t[1] <= 32768)
                if b["btype"] == 2:
                    assert len(b["ll_lens"]) == b["hlit"] and len(b["d_lens"]) == b["hdist"] and 4 <= b["hclen"] <= 19
                    assert deflate_writer.kraft(b["ll_lens"]) == 32768  # zlib's literal/length codes are complete
    assert seen == ({0, 1} if strategy == zlib.Z_FIXED else {0, 1, 2})  # the empty stored block of the full flush


def test_tokens_of_the_spec_corpus():
    """What zlib never writes: incomplete one-code distance trees, 15-bit codes, 284 + 31 for length 258, runs across the
    HLIT / HDIST boundary, several block types in one stream, bytes behind the final block."""
    n = 0
    for m in deflate_writer.spec_corpus():
        if m.status != deflate_writer.OK:
            continue
        blocks, used = deflate_tokens.read(m.payload)
        assert deflate_tokens.replay(blocks) == m.expect == zlib.decompressobj(-15).decompress(m.payload), m.name
        assert used <= len(m.payload)
        n += 1
    assert n > 200
