#!/usr/bin/env python3
"""tests/golden/tex_<name>_rows64.png — the first 64 rows of the reference's two 2048 x 2048 texture assets (`bananaDiffuse.png`,
RGBA; `toasterBaseColor.png`, RGB) as DATA fixtures for tests/test_texture_io.py.  The rows' filtered scanline bytes (filter type
byte + filtered samples, exactly as the asset stores them) are re-compressed into a PNG of height 64, split into 8 KiB IDAT chunks:
row 0 of a PNG is filtered against zeros, so the crop decodes to the asset's own first 64 rows.  Run once where the reference
tree exists:

    python tools/make_texture_crops.py "<reference>/FYPRayTracer/Assets/3D Models/Test"
"""
import struct
import sys
import zlib
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
ROWS = 64
NAMES = ("bananaDiffuse.png", "toasterBaseColor.png")


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def crop(src: Path, rows: int) -> bytes:
    raw = src.read_bytes()
    pos, idat, hdr = 8, b"", None
    while pos < len(raw):
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", raw[pos + 8:pos + 21])
        elif kind == b"IDAT":
            idat += raw[pos + 8:pos + 8 + n]
        pos += 12 + n
    w, _h, depth, ctype, comp, filt, interlace = hdr
    assert depth == 8 and ctype in (2, 6) and interlace == 0, hdr
    need = rows * (1 + w * {2: 3, 6: 4}[ctype])
    part = zlib.decompressobj().decompress(idat, need)
    assert len(part) == need
    z = zlib.compress(part, 9)
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, rows, depth, ctype, comp, filt, 0))
    for i in range(0, len(z), 8192):
        out += _chunk(b"IDAT", z[i:i + 8192])
    return out + _chunk(b"IEND", b"")


def main():
    src_dir = Path(sys.argv[1])
    for name in NAMES:
        out = ROOT / "tests" / "golden" / f"tex_{Path(name).stem}_rows{ROWS}.png"
        out.write_bytes(crop(src_dir / name, ROWS))
        print(f"{out}: {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
