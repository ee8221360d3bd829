"""The marshalling of zgpu.py's device-resident calls, without a GPU and without loading the library: the argument arrays, the conversion
of result records, and the keys of the statistics getters against the enumerators the C++ names their slots by."""
import os
import re

import pytest

import zgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_argument_arrays_and_length_check():
    for vals in ([], [0x7F0012345678], [0x1000, 0, 2 ** 64 - 1]):
        n = len(vals)
        p, s = zgpu._ptr_array(vals), zgpu._size_array(vals)
        assert len(p) == len(s) == max(n, 1)
        assert [p[i] for i in range(n)] == [v or None for v in vals]          # (0 reads back as NULL)
        assert [s[i] for i in range(n)] == vals
    assert zgpu._ptr_array([])[0] is None and zgpu._size_array([])[0] == 0
    assert zgpu._slots([0, 1, 256, 257]) == ([0, 0, 256, 512], 1024) and zgpu._slots([]) == ([], 0)
    zgpu._one_per("some_call", 3, [1, 2, 3], None, (4, 5, 6))
    zgpu._one_per("some_call", 0)
    for lists in (([1, 2],), ([1, 2, 3], None, [1, 2, 3, 4])):
        with pytest.raises(ValueError, match="some_call"):
            zgpu._one_per("some_call", 3, *lists)


def _fill(r, base, status):
    """distinct values in every field of a zgpu_entry_result"""
    r.written, r.status, r.nframes, r.checksums = (base << 33) + 1, status, base + 2, base + 3
    r.checksum_mismatches, r.checksum_from_data, r.calculated_checksum = base + 4, 0xF0000000 + base, 0xE0000000 + base


def _entry_fields(e, base, status):
    return (e.written, e.status, e.nframes, e.checksums, e.checksum_mismatches, e.checksum_from_data, e.calculated_checksum) == (
        (base << 33) + 1, status, base + 2, base + 3, base + 4, 0xF0000000 + base, 0xE0000000 + base)


def test_result_records_become_objects_field_for_field():
    statuses = [0, zgpu.E_CHECKSUM_MISMATCH, -5]           # (a failed entry is converted like any other: nothing is filtered)
    n = len(statuses)
    plain, dev, rng = (zgpu.EntryResultC * 4)(), (zgpu.DeviceEntryResultC * 4)(), (zgpu.RangeResultC * 4)()
    for i, st in enumerate(statuses):
        _fill(plain[i], 10 * i, st)
        _fill(dev[i].r, 100 + 10 * i, st)
        dev[i].checksums_unverified, dev[i].first_hashed = 100 + 10 * i + 7, 100 + 10 * i + 8
        _fill(rng[i].d.r, 200 + 10 * i, st)
        rng[i].d.checksums_unverified, rng[i].d.first_hashed = 200 + 10 * i + 7, 200 + 10 * i + 8
        for k, name in enumerate(zgpu.Seek.FIELDS):
            setattr(rng[i].seek, name, 1000 * (i + 1) + k)
    for arr in (plain, dev, rng):
        assert zgpu._results(arr, 0) == [] and len(zgpu._results(arr, n)) == n          # (the array may be longer than the call's n)
    for i, (st, e) in enumerate(zip(statuses, zgpu._results(plain, n))):
        assert type(e) is zgpu.EntryResult and _entry_fields(e, 10 * i, st) and not hasattr(e, "data")
    for arr, base in ((dev, 100), (rng, 200)):
        for i, (st, e) in enumerate(zip(statuses, zgpu._results(arr, n))):
            b = base + 10 * i
            assert type(e) is zgpu.DeviceEntryResult and _entry_fields(e, b, st)
            assert (e.checksums_unverified, e.first_hashed) == (b + 7, b + 8)
    for i in range(n):
        s = zgpu.Seek(rng[i].seek)
        assert s.key() == tuple(1000 * (i + 1) + k for k in range(11))
        assert (s.open_ended, s.broken, s.nothing) == (bool(s.flags & 1), bool(s.flags & 2), bool(s.flags & 4))


def _snake(name):
    return re.sub(r"(?<!^)([A-Z])", r"_\1", name).lower()


@pytest.mark.parametrize("getter, prefix", [("frames_dict_stats", "kDictStat"), ("frames_device_stats", "kDevStat"),
                                            ("frames_device_src_stats", "kSrcStat"), ("frames_index_stats", "kIndexStat"),
                                            ("ranges_stats", "kRangeStat")])
def test_stats_keys_are_the_enumerators(getter, prefix):
    text = open(os.path.join(ROOT, "zstd-rs_amd", "csrc", "zg_capi_int.h")).read()
    lists = [m for m in re.findall(r"enum\s*\{([^}]*)\}", text) if prefix in m]
    assert len(lists) == 1
    names = re.findall(r"\b%s(\w+)" % prefix, lists[0])
    assert names[-1] == "Count" and len(set(names)) == len(names)
    fn, ctype, keys = zgpu._STATS["Context." + getter]
    assert list(keys) == [_snake(k) for k in names[:-1]]
    assert fn == "zgpu_debug_" + getter and fn in zgpu.EXPORTS and callable(getattr(zgpu.Context, getter))
