"""What the GPU tests of the device-resident calls share: destination arenas and source tensors in device memory with sentinels and guard
regions, raw HIP allocations, the oracle's verdict on one entry, and the keys results are compared by."""
import ctypes as C

import torch   # (before the library is loaded: the process must run on one HIP runtime, Context.decode_frames_to_tensors)

MAGIC = (0xFD2FB528).to_bytes(4, "little")
SENT = 0xA5
GUARD = 256
ALL = 1 << 40                                      # hash_max: every frame hashed


def xxh64(b):
    import oracle
    return oracle.lib().zor_xxh64(b, len(b), 0)


def xxh32(b):
    return xxh64(b) & 0xFFFFFFFF


def oracle_alone(z, cap, dict_raw=None):
    import oracle
    d = oracle.FrameDecoder()
    if dict_raw is not None:
        d.add_dict(dict_raw)
    return d.decode_all(z, cap)


def entry_key(r):
    return (r.status, r.written, r.nframes, r.checksums, r.checksum_mismatches, r.checksum_from_data, r.calculated_checksum)


def full_key(r):
    return entry_key(r) + (r.checksums_unverified, r.first_hashed)


class Arena:
    """slots of caps[i] bytes in one device tensor full of the sentinel; slot i starts at offset shifts[i] (default 0) from a 256-byte aligned
    address, with at least GUARD bytes of sentinel on both sides"""

    def __init__(self, caps, shifts=None):
        self.caps = list(caps)
        self.offs, at = [], GUARD
        for i, c in enumerate(self.caps):
            at = (at + 255) & ~255
            self.offs.append(at + (shifts[i] if shifts else 0))
            at = self.offs[-1] + c + GUARD
        self.t = torch.full((at + GUARD,), SENT, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert self.t.data_ptr() % 256 == 0
        self.ptrs = [self.t.data_ptr() + o for o in self.offs]

    def check(self, plains):
        """plains[i]: what slot i must start with, or None if it must be untouched"""
        torch.cuda.synchronize()
        got = self.t.cpu().numpy().tobytes()
        want = bytearray([SENT]) * len(got)
        for o, c, p in zip(self.offs, self.caps, plains):
            if p is not None:
                assert len(p) <= c
                want[o:o + len(p)] = p
        if got != bytes(want):
            for i, (o, c, p) in enumerate(zip(self.offs, self.caps, plains)):
                lo, hi = o - GUARD, o + c + GUARD
                assert got[lo:hi] == bytes(want[lo:hi]), "slot %d (cap %d, %s) or its guards" % (i, c, "untouched" if p is None else len(p))
            assert False, "bytes between the slots changed"


def _packed(entries, shifts):
    """(offsets, host image): entry j starts shifts[j] bytes behind a 32-byte boundary, the bytes between entries are 0x3C"""
    offs, at = [], 0
    for j, z in enumerate(entries):
        at = ((at + 31) & ~31) + (shifts[j] if shifts else 0)
        offs.append(at)
        at += len(z)
    host = bytearray([0x3C]) * at
    for o, z in zip(offs, entries):
        host[o:o + len(z)] = z
    return offs, bytes(host)


class Sources:
    """the entries in ONE torch device tensor: entry j starts shifts[j] bytes behind a 32-byte boundary (default 0), other bytes between them
    are a sentinel the decoder must never need; the last entry ends with the tensor"""

    def __init__(self, entries, shifts=None):
        self.offs, host = _packed(entries, shifts)
        self.host = host or b"\x3C"
        self.t = torch.frombuffer(bytearray(self.host), dtype=torch.uint8).to("cuda:0")
        torch.cuda.synchronize()
        self.lens = [len(z) for z in entries]
        self.ptrs = [self.t.data_ptr() + o if n else 0 for o, n in zip(self.offs, self.lens)]

    def unchanged(self):
        torch.cuda.synchronize()
        return self.t.cpu().numpy().tobytes() == self.host


class RawDevice:
    """n bytes from the HIP runtime itself (hipMalloc through the one runtime the process has loaded): an allocation whose end is the
    end the runtime knows, which a torch tensor's — a piece of the caching allocator's block — is not"""

    def __init__(self, data):
        paths = sorted(set(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
        assert len(paths) == 1, paths
        self.hip = C.CDLL(paths[0])
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), len(data)) == 0
        self.ptr, self.n, self.data = p.value, len(data), bytes(data)
        assert self.hip.hipMemcpy(self.ptr, self.data, self.n, 1) == 0

    def read(self):
        out = C.create_string_buffer(self.n)
        assert self.hip.hipMemcpy(out, self.ptr, self.n, 2) == 0
        return out.raw

    def free(self):
        if self.ptr:
            self.hip.hipFree(self.ptr)
            self.ptr = None


class RawSources:
    """entries back to back (shifted) in one RawDevice allocation; the last entry ends flush with the allocation"""

    def __init__(self, entries, shifts):
        self.offs, host = _packed(entries, shifts)
        self.dev = RawDevice(host)
        self.lens = [len(z) for z in entries]
        self.ptrs = [self.dev.ptr + o if n else 0 for o, n in zip(self.offs, self.lens)]
        assert self.offs[-1] + self.lens[-1] == self.dev.n and self.lens[-1] > 0

    def unchanged(self):
        return self.dev.read() == self.dev.data

    def free(self):
        self.dev.free()
