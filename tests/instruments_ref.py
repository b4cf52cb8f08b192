"""Host references for the library's device instruments (include/cronsun_gpu.h:
cg_checksum_device, cg_node_checksum_enqueue), written from the header's
definition and from nothing in the library:

    checksum(v, first_index, add) =
        sum_i mix(((v[i] + add) mod 2^64) XOR mix(((first_index + i) mod 2^64) * GOLDEN mod 2^64))  mod 2^64

mix = the splitmix64 finaliser, int32 elements sign-extended to 64 bits first.
checksum_ref is the definition in plain Python integers; checksum_ref_np the
same in numpy uint64 for arrays of millions of elements (the two are compared
in tests/test_instruments_ref.py)."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MUL1 = 0xBF58476D1CE4E5B9
MUL2 = 0x94D049BB133111EB

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def mix(x):
    x ^= x >> 30
    x = x * MUL1 & M64
    x ^= x >> 27
    x = x * MUL2 & M64
    return x ^ (x >> 31)


def _signed(x, elem_bytes):
    """One element as the signed integer its elem_bytes-wide two's complement word holds."""
    bits = 8 * elem_bytes
    x = int(x) & ((1 << bits) - 1)
    return x - (1 << bits) if x >> (bits - 1) else x


def checksum_ref(values, elem_bytes, first_index=0, add=0):
    if elem_bytes not in (4, 8):
        raise ValueError("elem_bytes must be 4 or 8")
    acc = 0
    for i, v in enumerate(values):
        x = (_signed(v, elem_bytes) + int(add)) & M64
        acc += mix(x ^ mix(((int(first_index) + i) & M64) * GOLDEN & M64))
    return acc & M64


def _mix_np(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(MUL1)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(MUL2)
    return x ^ (x >> np.uint64(31))


def checksum_ref_np(values, elem_bytes, first_index=0, add=0):
    if elem_bytes not in (4, 8):
        raise ValueError("elem_bytes must be 4 or 8")
    v = np.asarray(values)
    if v.dtype != (np.int32 if elem_bytes == 4 else np.int64):
        raise ValueError("values must be an int32 (elem_bytes 4) or int64 (elem_bytes 8) array")
    with np.errstate(over="ignore"):
        x = v.astype(np.int64).view(np.uint64) + np.uint64(int(add) & M64)
        pos = np.arange(len(v), dtype=np.uint64) + np.uint64(int(first_index) & M64)
        return int(_mix_np(x ^ _mix_np(pos * np.uint64(GOLDEN))).sum(dtype=np.uint64))


def node_list_checksum_ref(time, rule):
    """cg_node_checksum_enqueue's pair for one node's list: positions relative
    to the list's start, nothing added."""
    return checksum_ref(time, 8), checksum_ref(rule, 4)


def node_list_checksum_ref_np(time, rule):
    return (checksum_ref_np(np.asarray(time, dtype=np.int64), 8),
            checksum_ref_np(np.asarray(rule, dtype=np.int32), 4))
