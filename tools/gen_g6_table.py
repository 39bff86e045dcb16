"""Prints the power-of-ten table of msweep_amd/csrc/g6_format.hpp: for k = -310 ... 345 the pair (P, q) with
P = floor(10^k / 2^q), 2^63 <= P < 2^64, in exact integer arithmetic.  tests/test_g6_format_cpu.py recomputes every
entry with fractions.Fraction.

    python tools/gen_g6_table.py > table.txt      # the lines between the BEGIN / END TABLE marks of the header
"""
KMIN, KMAX = -310, 345


def entry(k):
    if k >= 0:
        d = 10 ** k
        bl = d.bit_length()
        return (d << (64 - bl), bl - 64) if bl <= 64 else (d >> (bl - 64), bl - 64)
    d = 10 ** -k
    bl = d.bit_length()
    return (1 << (63 + bl)) // d, -(63 + bl)


if __name__ == "__main__":
    for k in range(KMIN, KMAX + 1):
        p, q = entry(k)
        assert 1 << 63 <= p < 1 << 64
        print("    {0x%016xull, %d},  // 1e%d" % (p, q, k))
