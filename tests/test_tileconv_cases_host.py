"""The table of tests/tileconv_cases.py against the host side of the dispatch: every row takes the kernel it names, every route of the tile family is reached
(forward, and data gradient where the kernel serves one), on both libraries.  No GPU."""
import tileconv_cases as TC


def test_every_row_takes_its_kernel_and_every_route_is_reached():
    routes = TC.check_coverage()
    print('\n'.join(routes))
    assert len(routes) == 18


def test_the_f16_library_routes_the_forward_rows_alike():
    TC.check_coverage_f16()


def test_geometry_of_the_special_rows():
    # the data gradient of a reflect-padded layer runs over the explicitly padded extent
    r = [r for r in TC.ALL_ROWS if r.pad_mode == TC.RF and r.direction == 'dgrad'][0]
    _, n, hi, wi, _, ho, wo, _, hq, wq = TC.geometry(r)
    assert (hi, wi) == (r.H, r.W) and (ho, wo) == (hq, wq) == (r.H + 2 * r.pad, r.W + 2 * r.pad)
    # more tiles than conv_c4_patch's grid cap of 512 / (Co / 64) workgroups: a persistent workgroup takes a second tile
    n, h, w = TC.C4_CAPPED
    assert n * (h // 4) * (w // 64) == 513 and h % 4 == 0 and w % 64 == 0
    # the 8-phase rows at the edge of the 224-workgroup rule, and the ragged one
    assert 7 * 64 * 64 // 256 * (512 // 256) == 224 and (5 * 60 * 100) % 256 != 0 and (60 * 100) % 256 != 0
