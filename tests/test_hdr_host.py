"""host/hdr_decode.js, the Radiance .hdr reader behind `render_cli.js --env`, without a GPU: tiny RGBE files written here — flat
scanlines, and new-style run-length scanlines holding a run and a literal span — decoded through node and compared exactly with the
RGBE-to-float formula; truncated files are errors, not crashes."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "wgpu-path-tracing_amd", "host")

pytestmark = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")

SCRIPT = ("const fs = require('fs'); const {decodeHDR} = require(process.argv[1]);"
          "try { const r = decodeHDR(fs.readFileSync(process.argv[2]));"
          " console.log(JSON.stringify({width: r.width, height: r.height, data: Buffer.from(r.data.buffer, r.data.byteOffset, r.data.byteLength).toString('base64')})); }"
          "catch (e) { console.log(JSON.stringify({error: String(e.message)})); }")


def decode(path):
    out = subprocess.run(["node", "-e", SCRIPT, os.path.join(HOST, "hdr_decode.js"), str(path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout)
    if "error" in r:
        return r
    import base64
    r["data"] = np.frombuffer(base64.b64decode(r["data"]), np.float32).reshape(r["height"], r["width"], 4)
    return r


def rgbe_to_float(rgbe):
    """(H, W, 4) uint8 -> (H, W, 4) float32, alpha 1: (r, g, b) 2^(e - 136), zero when e = 0"""
    e = rgbe[..., 3].astype(np.int32)
    f = np.where(e == 0, 0.0, np.ldexp(1.0, e - 136))
    out = np.ones(rgbe.shape, np.float32)
    out[..., :3] = (rgbe[..., :3].astype(np.float64) * f[..., None]).astype(np.float32)
    return out


HEADER = b"#?RADIANCE\n# written by a test\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n"


def texels(w, h, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    t[..., 3] = rng.integers(120, 140, (h, w))
    t[0, 0] = (200, 100, 50, 0)                                  # e = 0: black whatever the mantissas say
    return t


def rle_channel(vals):
    """one channel of a scanline: a run of the first 5 values' worth (made equal by the caller), the rest as literal spans"""
    out, x = bytearray(), 0
    while x < len(vals):
        n = 1
        while x + n < len(vals) and vals[x + n] == vals[x] and n < 127:
            n += 1
        if n >= 3:
            out += bytes([128 + n, vals[x]])
            x += n
        else:
            m = min(len(vals) - x, 5)
            out += bytes([m]) + bytes(vals[x:x + m])
            x += m
    return bytes(out)


def test_flat_scanlines(tmp_path):
    t = texels(8, 4, 1)
    p = tmp_path / "flat.hdr"
    p.write_bytes(HEADER + b"-Y 4 +X 8\n" + t.tobytes())
    r = decode(p)
    assert (r["width"], r["height"]) == (8, 4)
    assert np.array_equal(r["data"].view(np.uint32), rgbe_to_float(t).view(np.uint32))


def test_run_length_scanlines(tmp_path):
    t = texels(16, 4, 2)
    t[:, 3:9, 0] = 77                                            # a run in the red channel, literal spans around it
    t[:, :, 3] = 129                                             # the exponent channel is one long run
    t[0, 0, 3] = 0
    body = bytearray()
    for y in range(4):
        body += bytes([2, 2, 0, 16])
        for ch in range(4):
            enc = rle_channel(t[y, :, ch].tolist())
            body += enc
    assert any(b > 128 for b in body) and len(body) < t.nbytes + 4 * 4 * 5      # it holds runs
    p = tmp_path / "rle.hdr"
    p.write_bytes(HEADER + b"-Y 4 +X 16\n" + bytes(body))
    r = decode(p)
    assert (r["width"], r["height"]) == (16, 4)
    assert np.array_equal(r["data"].view(np.uint32), rgbe_to_float(t).view(np.uint32))


def test_truncated_and_foreign_files_are_errors(tmp_path):
    t = texels(8, 4, 3)
    whole = HEADER + b"-Y 4 +X 8\n" + t.tobytes()
    for name, blob in (("short", whole[:-5]), ("header_only", HEADER), ("no_signature", b"P6\n8 4\n255\n" + t.tobytes()),
                       ("other_orientation", HEADER + b"+Y 4 +X 8\n" + t.tobytes()),
                       ("rle_cut", HEADER + b"-Y 1 +X 16\n" + bytes([2, 2, 0, 16, 128 + 16, 9, 128 + 16]))):
        p = tmp_path / (name + ".hdr")
        p.write_bytes(blob)
        assert "error" in decode(p), name
