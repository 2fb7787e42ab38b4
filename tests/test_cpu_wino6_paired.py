"""The paired F(4x4,3x3) Winograd form (tune_wm 6 / tune_sc 32) on the host side: the library's resolve and argument checks and the
variant menu of ops.py (no GPU needed; nothing is launched)."""
import ctypes


def _desc(lib_mod, ptr, tune, n=8, h=50, w=80, cin=64, cout=64, splitk=0):
    d = lib_mod.ConvDesc()
    d.x = d.w = d.scale = d.shift = d.y = d.w_wino6 = ptr
    d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = n, h, w, cin, cout, 3, 1
    d.x_cs, d.y_cs = cin, cout
    d.tune_wm, d.tune_sc, d.tune_wn = tune
    d.splitk, d.splitk_ws = splitk, (ptr if splitk else None)
    return d


def test_paired_form_resolves_and_bad_combinations_are_refused():
    from centermask2_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 15) // 16 * 16
    for tv in ((6, 32, 1), (6, 32, 2)):                       # explicit variants come back unchanged
        v = (ctypes.c_int * 3)()
        assert lib.cmk_conv_resolve(ctypes.byref(_desc(_lib, ptr, tv)), 1, 0, v) == 0 and tuple(v) == tv
    # refused before anything is launched: unknown tune_sc, unknown geometry, split-K on the RoI geometry / uneven chunk counts
    for tv, splitk, what in (((6, 48, 1), 0, b"tune_sc"), ((6, 32, 3), 0, b"tune_wn"), ((6, 32, 2), 2, b"split-K"),
                             ((6, 64, 1), 2, b"split-K"), ((6, 32, 1), 8, b"split-K")):
        assert lib.cmk_conv2d_nhwc(ctypes.byref(_desc(_lib, ptr, tv, splitk=splitk)), None) != 0, tv
        assert what in lib.cmk_last_error(), (tv, lib.cmk_last_error())


def test_paired_form_is_on_the_menu():
    from centermask2_amd import ops
    for tv in ((6, 32, 1), (6, 32, 2), (6, 32, 1, 2), (6, 32, 1, 4), (6, 16, 1, 4), (6, 64, 1)):
        assert ops._variant_on_menu(tv), tv
    for tv in ((6, 32, 3), (6, 48, 1), (6, 64, 1, 2)):
        assert not ops._variant_on_menu(tv), tv
    from centermask2_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 15) // 16 * 16

    def plan(tv, aff=False, **shape):
        d = _desc(_lib, ptr, tv, **shape)
        if aff:
            d.in_scale = d.in_shift = ptr
        name, flops = ctypes.create_string_buffer(96), ctypes.c_double()
        assert lib.cmk_conv_plan(ctypes.byref(d), 1, name, len(name), ctypes.byref(flops), None) == 0, lib.cmk_last_error()
        return name.value.decode(), flops.value

    assert plan((6, 32, 1), aff=True)[0] == "conv_wino6p_kernel<true, 0>"
    assert plan((6, 32, 2), h=14, w=14)[0] == "conv_wino6p_kernel<false, 1>"
    assert plan((6, 16, 1))[0] == "conv_wino6_kernel<false, 0>"
    # two cout tiles per workgroup: an odd last pair still executes two tiles' MFMAs
    f16 = plan((6, 16, 1), n=8, h=100, w=160, cin=256, cout=80)[1]
    f32 = plan((6, 32, 1), n=8, h=100, w=160, cin=256, cout=80)[1]
    assert f32 == f16 * 4 / 3
