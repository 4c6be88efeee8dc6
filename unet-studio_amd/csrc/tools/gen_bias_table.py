#!/usr/bin/env python3
"""Writes csrc/bias_table.h: T[j] = the float32 nearest to 2^(j / 4096), j = 0..4095 (include/unet_bias.h, Apply).  Each entry is the
float64 exp2 rounded to float32, then PROVEN nearest in integer arithmetic: with m the entry's 24-bit mantissa (T = m * 2^-23), the
two midpoints (2m - 1) * 2^-24 and (2m + 1) * 2^-24 raised to the 4096th power must bracket 2^j.  Run by hand when the definition
changes; the build only reads the header."""
import math
import os
import struct


def entry(j):
    f = struct.unpack("<f", struct.pack("<f", math.pow(2.0, j / 4096.0)))[0]
    m = int(f * (1 << 23))
    assert m * 2.0 ** -23 == f and (1 << 23) <= m < (1 << 24)
    target = 1 << (j + 24 * 4096)                                   # 2^j * (2^24)^4096
    assert (2 * m - 1) ** 4096 < target < (2 * m + 1) ** 4096 or (j == 0 and m == 1 << 23), j
    return f


def main():
    rows = [entry(j) for j in range(4096)]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bias_table.h")
    with open(out, "w") as fh:
        fh.write("// T[j] = the float32 nearest to 2^(j / 4096) (include/unet_bias.h, Apply), written by tools/gen_bias_table.py, which proves\n"
                 "// every entry nearest in integer arithmetic.  Hexadecimal literals, the 23 mantissa bits in six digits: the bits are what is written.\n"
                 "#pragma once\n\n#define BIAS_TABLE_VALUES \\\n")
        for r in range(0, 4096, 8):
            fh.write("    " + " ".join("0x1.%06xp+0f," % ((int(v * (1 << 23)) - (1 << 23)) << 1) for v in rows[r:r + 8]) + (" \\\n" if r + 8 < 4096 else "\n"))


if __name__ == "__main__":
    main()
