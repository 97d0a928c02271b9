"""Plain-loop restatement of the run-length mask format, for the tests: it imports nothing from the package and
uses no array library.  A mask is a list of H rows of W numbers (non-zero = set).

  pixel order   column-major, p = x H + y
  run list      c[0] zeros (possibly 0 long), c[1] ones, alternating; canonical: every later run >= 1 long, the sum H W
  packed form   ceil(H W / 64) words, bit k of word j = ROW-major pixel 64 j + k, the bits past H W zero; area = the set pixels
"""


def encode(mask):
    """One pixel at a time in column-major order: a run ends where the value changes; the first run counts zeros."""
    H, W = len(mask), len(mask[0])
    counts, value, run = [], 0, 0
    for x in range(W):
        for y in range(H):
            v = 1 if mask[y][x] else 0
            if v != value:
                counts.append(run)
                value, run = v, 0
            run += 1
    counts.append(run)
    return counts


def check(counts, H, W):
    """Why a decoder refuses the list, or None."""
    if len(counts) == 0:
        return "empty"
    for c in counts:
        if c < 0:
            return "negative"
    total = 0
    for c in counts:
        total += c
    return None if total == H * W else "sum"


def decode(counts, H, W):
    """-> H rows of W values 0 / 1; zero-length runs are allowed anywhere."""
    assert check(counts, H, W) is None
    mask = [[0] * W for _ in range(H)]
    p = 0
    for i, c in enumerate(counts):
        for _ in range(c):
            if i % 2 == 1:
                mask[p % H][p // H] = 1
            p += 1
    return mask


def packed(mask):
    """-> (words as Python ints in [0, 2^64), area), bit by bit."""
    H, W = len(mask), len(mask[0])
    words = [0] * ((H * W + 63) // 64)
    area = 0
    for y in range(H):
        for x in range(W):
            if mask[y][x]:
                p = y * W + x
                words[p // 64] |= 1 << (p % 64)
                area += 1
    return words, area


def signed64(word):
    """A word as the int64 a tensor holds."""
    return word - (1 << 64) if word >= 1 << 63 else word
