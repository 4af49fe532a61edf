"""CPU (no GPU): group copies -- one packed copy for linears that are always launched together (tce_w4a16_prepack_group; csrc/w4a16_mfma_layout.hpp: packed_view).

  * the member-offset arithmetic against the single-linear arithmetic of w4a16_mfma_layout.hpp applied to the row-concatenated linear (tests/host/test_group_pack.cc,
    compiled with g++ and run here);
  * the byte count of the C ABI: that of tce_w4a16_prepack_bytes for the concatenation; members with N % 16 != 0, differing K or differing group size are refused
    (0 bytes; tce_w4a16_prepack_group: TCE_ERR_UNSUPPORTED_SHAPE before any HIP call -- host buffers stand in for device pointers and are never dereferenced);
  * descriptors with 0 / 0 in the two fields are what they were; fields that describe no slice of a copy are refused."""
import ctypes as C
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from tinychatengine_amd import build as B
    B.build()
    from tinychatengine_amd import capi
    return capi


def test_member_offsets_match_the_concatenated_linear(tmp_path):
    exe = tmp_path / "test_group_pack"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(REPO, "tinychatengine_amd", "csrc"),
                           os.path.join(REPO, "tests", "host", "test_group_pack.cc"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "group pack ok" in r.stdout, r.stdout + r.stderr


_keep = []


def _desc(capi, n, k, g, **kw):
    buf = (C.c_uint8 * 64)()  # never dereferenced: every check below fails or answers before a HIP call
    _keep.append(buf)
    p = C.addressof(buf)
    return capi.W4A16Desc(M=1, N=n, K=k, group_size=g, A=p, qweight=p, scales=p, zeros=p, C=p, **kw)


def _arr(capi, descs):
    return (capi.W4A16Desc * len(descs))(*descs)


@pytest.mark.parametrize("ns,k,g", [((16, 32), 128, 128), ((48, 16, 1024), 1152, 64), ((1024, 48, 32, 16), 4096, 32), ((4096, 1024, 1024), 4096, 128), ((14336, 14336), 4096, 128)])
def test_group_bytes_are_those_of_the_concatenation(capi, ns, k, g):
    L = capi.lib()
    got = int(L.tce_w4a16_prepack_group_bytes(_arr(capi, [_desc(capi, n, k, g) for n in ns]), len(ns)))
    assert got == int(L.tce_w4a16_prepack_bytes(sum(ns), k, g)) and got > 0
    # parts in the order words, ..., scales, zero points: the copy is at least the members' own copies less their per-part padding
    assert got <= sum(int(L.tce_w4a16_prepack_bytes(n, k, g)) for n in ns)


@pytest.mark.parametrize("members", [
    [(24, 128, 128), (32, 128, 128)],      # N % 16 != 0
    [(32, 128, 128), (40, 128, 128)],
    [(32, 128, 128), (32, 256, 128)],      # differing K
    [(32, 256, 128), (32, 256, 64)],       # differing group size
    [(32, 192, 64), (32, 192, 64)],        # K % 128 != 0: no packed form at all
])
def test_members_that_cannot_share_a_copy_are_refused(capi, members):
    L = capi.lib()
    arr = _arr(capi, [_desc(capi, *m) for m in members])
    assert int(L.tce_w4a16_prepack_group_bytes(arr, len(members))) == 0
    dst = (C.c_uint8 * 512)()
    aligned = (C.addressof(dst) + 255) & ~255
    assert L.tce_w4a16_prepack_group(arr, len(members), C.c_void_p(aligned), None) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    L.tce_reset_last_error()


def test_count_and_null_arguments(capi):
    L = capi.lib()
    arr = _arr(capi, [_desc(capi, 32, 128, 128)] * 5)
    assert int(L.tce_w4a16_prepack_group_bytes(arr, 5)) == 0 and int(L.tce_w4a16_prepack_group_bytes(arr, 0)) == 0
    assert int(L.tce_w4a16_prepack_group_bytes(arr, 1)) == int(L.tce_w4a16_prepack_bytes(32, 128, 128))
    assert L.tce_w4a16_prepack_group(arr, 5, C.c_void_p(256), None) == capi.TCE_ERR_BAD_ARG
    assert L.tce_w4a16_prepack_group(arr, 2, None, None) == capi.TCE_ERR_BAD_ARG
    L.tce_reset_last_error()


def test_zero_fields_behave_as_before_and_bad_fields_are_refused(capi):
    packed = 1 << 20  # (a 256-byte aligned stand-in: describe launches nothing)
    own = _desc(capi, 4096, 4096, 128, prepacked=packed, flags=capi.TCE_W4_ZERO_POINT_IS_8)
    assert own.reserved == 0 and own.reserved2 == 0
    assert capi.describe_dispatch(own) == "gemv-i8 rows-per-pass=1 group=128"
    member = _desc(capi, 1024, 4096, 128, prepacked=packed, flags=capi.TCE_W4_ZERO_POINT_IS_8, reserved=256, reserved2=6144)
    assert capi.describe_dispatch(member) == "gemv-i8 rows-per-pass=1 group=128 group-copy first-tile=256 rows=6144"
    buf = C.create_string_buffer(256)
    L = capi.lib()
    for bad in (dict(reserved=1, reserved2=0),                       # a first tile without a copy
                dict(reserved=0, reserved2=6144, prepacked=None),    # a copy's rows without a copy
                dict(reserved=321, reserved2=6144),                  # rows [5136, 6160) of a 6144-row copy
                dict(reserved=0, reserved2=6150),                    # a copy that is no whole number of tiles
                dict(reserved=-1, reserved2=6144)):
        d = _desc(capi, 1024, 4096, 128, **{"prepacked": packed, "flags": capi.TCE_W4_ZERO_POINT_IS_8, **bad})
        assert L.tce_w4a16_describe_dispatch(C.byref(d), buf, 256) == capi.TCE_ERR_BAD_ARG, bad
    L.tce_reset_last_error()
