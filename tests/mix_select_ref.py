"""numpy restatement of rgda_mix_select_classes (include/rgda_hip.h), the DACS draw: of the classes that occur in a source
label map, the (P + 1) // 2 of smallest rank.  Integer work only: every comparison against it is exact."""
import numpy as np

TABLE_COLS = 8


def select_classes(label_s, ranks, ignore_label=-1):
    """label_s int64 [N][H][W] (or [N][1][H][W]), ranks uint8 [N][C] -> (class_bits uint32 [N], flag).  Equal ranks are
    ordered by class id, a rank at or above C never selects its class; the flag is 1 where a label is neither in [0, C)
    nor ignore_label."""
    ranks = np.asarray(ranks)
    n, C = ranks.shape
    l = np.asarray(label_s).reshape(n, -1)
    bits = np.zeros(n, np.uint32)
    for i in range(n):
        present = [c for c in range(C) if (l[i] == c).any()]
        k = (len(present) + 1) // 2
        order = sorted(present, key=lambda c: (int(ranks[i][c]), c))
        for c in order[:k]:
            if int(ranks[i][c]) < C:
                bits[i] |= np.uint32(1 << c)
    flag = int((((l < 0) | (l >= C)) & (l != ignore_label)).any())
    return bits, flag


def classes_of(bits, C):
    return [c for c in range(C) if (int(bits) >> c) & 1]


def table_rows(n, class_bits=0, box=(0, 0, 0, 0)):
    """The table rgda_mix_write_table writes: every row {class_bits, y0, y1, x0, x1, 0, 0, 0} (int32)."""
    row = np.array([class_bits, *box, 0, 0, 0], np.int64).astype(np.uint32).view(np.int32)      # bit 31 is a class too
    return np.tile(row, (n, 1))
