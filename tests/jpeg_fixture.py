"""Fixture G22 (tests/golden/g22_jpeg.npz, written by tests/golden/make_jpeg_golden.py) as the JPEG tests read it."""
import json
import os

import numpy as np

from grit_amd.ops import jpeg
from tests.conftest import GOLDEN

LISTED_SIZES = [(1, 1), (2, 3), (3, 5), (5, 4), (8, 8), (9, 17), (16, 16), (17, 33), (24, 40), (31, 47), (33, 18)]  # (w, h)


class Fixture(object):
    def __init__(self):
        z = np.load(os.path.join(GOLDEN, 'g22_jpeg.npz'))
        self.meta = json.loads(str(z['meta']))
        self.data = [z['f%d' % i].tobytes() for i in range(len(self.meta))]
        self.pixels = [z['p%d' % i] for i in range(len(self.meta))]
        self.accepted = [i for i, m in enumerate(self.meta) if m['accepted']]
        self.refused = [i for i, m in enumerate(self.meta) if not m['accepted']]
        self._items = {}

    def item(self, i):
        """The file entropy-decoded (once; shared and left unchanged)."""
        if i not in self._items:
            it = jpeg.probe(self.data[i])
            assert it is not None and jpeg.entropy(it) is it
            self._items[i] = it
        return self._items[i]

    def index(self, name):
        return [m['name'] for m in self.meta].index(name)

    def colour(self, size, sampling, restart):
        """Accepted three-component files of that (w, h) and (hmax, vmax), with (True) or without (False) restart markers."""
        return [i for i in self.accepted
                if (self.meta[i]['width'], self.meta[i]['height'], self.meta[i]['ncomp']) == size + (3,)
                and (self.meta[i]['hmax'], self.meta[i]['vmax']) == sampling and (self.meta[i]['restart'] > 0) == restart]


def with_quant(data, value):
    """The file with every entry of every quantisation table replaced by `value`."""
    data, pos = bytearray(data), 2
    while data[pos + 1] != 0xDA:
        n = (data[pos + 2] << 8) | data[pos + 3]
        if data[pos + 1] == 0xDB:
            for at in range(pos + 4, pos + 2 + n, 65):
                data[at + 1:at + 65] = bytes([value]) * 64
        pos += 2 + n
    return bytes(data)
