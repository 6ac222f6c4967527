"""The comparator of tests/test_gpu_fusion6.py can fail (no GPU): on that test's own shapes, plane counts and inputs it accepts r32,
the fp32 evaluation of the reference on the CPU, against r64, and rejects every float64 mutant below wherever the mutation changes
anything -- with the values of c that the GPU measurement fixed (fusion6_ref.C).

  tap dropped       the weakest Gaussian tap missing in the last valid column; in the last valid row: the SSIM tile sums, the target
                    maps and dpred (structural alone, with the L1 term, with the L2 term)
  row 17 twice      the map row at tile-local row 17 of the column pass counted twice in its tile's SSIM partial (changes something
                    once the valid map has a row 7)
  no apron          the gradient of every tile formed from its own part of the derivative maps alone (changes something once the image
                    has more than one tile)
  frame 0           the target maps of frame 0 read whatever the frame index is
  planes exchanged  the G*t and G*t^2 planes of the table exchanged: the table itself, and dpred of a step that reads it
  g_ssim            formed with H*W instead of (H-10)*(W-10)
  L2T               the L2T form given the L1 sign term: with the form's own g_l1 (0 for Fusion1) and with g_l2
Mutants run on the suite's pair at every shape and plane count, and on the flat and the tied pair at three planes.  One exception, by
the nature of the input: the flat pair's SSIM map is 1 - O(1e-3) whatever the window, so a dropped tap moves its tile SUMS by less
than c E; there the tap mutants are rejected in dpred and in the target maps only.  Likewise its whole L2 pixel term (d ~ 1e-3) is of the
order of E of its structural gradient: the L2T form with no pixel term at all is rejected on the other two inputs only.
Also: the loss weights the reference uses are the library's (orn_loss_spec)."""
import ctypes

import pytest
import torch

import fusion6_ref as Q
import msssim_levels_ref as R

F64, F32 = Q.F64, Q.F32
torch.set_num_threads(min(16, torch.get_num_threads()))
ids = dict(ids=lambda s: 'x'.join(map(str, s)))


def test_loss_weights_are_the_librarys():
    import orn_amd
    from orn_amd import _build
    _build.build()
    L = orn_amd._lib.lib()
    for name, (lid, w1, w2, ws) in Q.LOSSES.items():
        w, kind = (ctypes.c_float * 3)(), ctypes.c_int()
        assert L.orn_loss_spec(lid, w, ctypes.byref(kind)) == 0, name
        assert list(w) == [ctypes.c_float(v).value for v in (w1, w2, ws)], name
        assert kind.value == (2 if name == 'Fusion10' else 1 if ws else 0), name


def rejected(kind, name, mut, r64, r32, changes=True):
    """the mutant differs from r64 exactly where it is expected to (elsewhere it is r64 up to float64 rounding), and the comparator
    rejects it there"""
    r = R.ratio(mut, r64, r32)
    assert (r > 1e-3) == changes, (kind, name, r)
    if changes:
        print(f'{kind:12s} {name}: ratio {r:.3g}')
        assert r > Q.C[kind], (kind, name, r)


def mutant_cases():
    for shape in Q.SHAPES:
        for B, Ch in Q.PLANES:
            yield pytest.param('pair', B * Ch, shape, id=f'pair-{B * Ch}-{shape[0]}x{shape[1]}')
        for kind in ('flat', 'tied'):
            yield pytest.param(kind, 3, shape, id=f'{kind}-3-{shape[0]}x{shape[1]}')


@pytest.mark.parametrize('planes', Q.PLANES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('shape', Q.SHAPES, **ids)
def test_comparator_accepts_fp32(shape, planes):
    H, W = shape
    P = planes[0] * planes[1]
    for kind in Q.KINDS:
        cs = Q.case(kind, P, H, W)
        r64, r32 = cs['ref'][F64], cs['ref'][F32]
        assert R.ratio(r32['part_ssim'], r64['part_ssim'], r32['part_ssim']) <= 1.0 <= Q.C['ssim part']
        assert R.ratio(r32['part_l1'], r64['part_l1'], r32['part_l1']) <= 1.0 <= Q.C['pix part']
        assert R.ratio(Q.dpred_ref(cs, 'SSIM', F32), Q.dpred_ref(cs, 'SSIM', F64), Q.dpred_ref(cs, 'SSIM', F32)) <= 1.0 <= Q.C['dpred struct']
        for loss in ('Fusion6', 'Fusion1'):
            assert R.ratio(Q.dpred_ref(cs, loss, F32), Q.dpred_ref(cs, loss, F64), Q.dpred_ref(cs, loss, F32)) <= 1.0 <= Q.C['dpred pixel']
        for a, b in zip(Q.target_maps(cs['t'], F32), Q.target_maps(cs['t'], F64)):
            assert R.ratio(a, b, a) <= 1.0 <= Q.C['tmaps']
        if kind == 'tied':
            m = Q.tied_mask(P, H, W)
            assert int(m.sum()) == (H * W + 1) // 2 and torch.equal(cs['p'][m], cs['t'][m])
            for dt in (F64, F32):
                assert bool((r64['l1'][m] == 0).all()) and bool((cs['ref'][dt]['l1'][~m] != 0).all())


@pytest.mark.parametrize('kind,P,shape', mutant_cases())
def test_comparator_rejects_mutants(kind, P, shape):
    H, W = shape
    cs = Q.case(kind, P, H, W)
    p, t, r64, r32 = cs['p'], cs['t'], cs['ref'][F64], cs['ref'][F32]
    tm64, tm32 = Q.target_maps(t, F64), Q.target_maps(t, F32)

    def dpreds(name, terms, losses=('SSIM', 'Fusion6', 'Fusion1'), changes=True):
        for loss in losses:
            rejected('dpred struct' if loss == 'SSIM' else 'dpred pixel', f'{name} {loss}', Q.combine(terms, loss), Q.dpred_ref(cs, loss, F64),
                     Q.dpred_ref(cs, loss, F32), changes)

    for where in ('col', 'row'):
        mut = Q.term_grads(p, t, F64, lambda x, y, w: R.maps_tap_dropped(where)(x, y, w)[0])
        if kind == 'flat':
            # p ~ t: numerator and denominator of the map lose the tap alike, the map stays 1 - O(1e-3) whatever the window and its
            # tile sums move by a few E only (measured 1.6 .. 7.3 E) -- nothing a sum can see; dpred and the target maps below do
            print(f'flat: tap {where} moves the SSIM sums by {R.ratio(Q.image_tile_sums(mut["map"], H, W), r64["part_ssim"], r32["part_ssim"]):.3g} E')
        else:
            rejected('ssim part', f'tap {where}', Q.image_tile_sums(mut['map'], H, W), r64['part_ssim'], r32['part_ssim'])
        dpreds(f'tap {where}', mut)
        for k, m in enumerate(Q.target_maps(t, F64, drop=where)):
            rejected('tmaps', f'tap {where} map {k}', m, tm64[k], tm32[k])
    rejected('ssim part', 'row 17 twice', Q.part_ssim_row17_twice(r64['map'], H, W), r64['part_ssim'], r32['part_ssim'], changes=H - 10 > 7)
    dpreds('no apron', Q.with_struct(r64, Q.struct_grad_without_apron(p, t)), changes=H > Q.TH or W > Q.TW)
    dpreds('planes exchanged', Q.with_struct(r64, Q.struct_grad_from(p, t, tm64[1], tm64[0])))
    assert R.ratio(Q.struct_grad_from(p, t, *tm64), r64['struct'], r32['struct']) < 1e-3        # the handed-in form itself is the reference
    dpreds('g_ssim', Q.with_struct(r64, r64['struct'] * ((H - 10) * (W - 10) / (H * W))))
    g_l1, g_l2, _ = Q.scales('Fusion1', P, H, W)
    sign = torch.sign(p.double() - t.double())
    assert g_l1 == 0.0
    for name, pix in (('L2T with its g_l1', g_l1 * sign), ('L2T with sign', g_l2 * sign)):
        if kind == 'flat' and pix.abs().max() == 0:
            # d ~ 1e-3: the whole L2 pixel term g_l2 d is of the order of E of the flat pair's structural gradient (measured 0.8 .. 5.2 E),
            # so its absence cannot show there; it does on the other two inputs
            print(f'flat: {name} moves dpred by {R.ratio(pix + 0.7 * r64["struct"], Q.dpred_ref(cs, "Fusion1", F64), Q.dpred_ref(cs, "Fusion1", F32)):.3g} E')
            continue
        rejected('dpred pixel', name, pix + 0.7 * r64['struct'], Q.dpred_ref(cs, 'Fusion1', F64), Q.dpred_ref(cs, 'Fusion1', F32))


@pytest.mark.parametrize('shape', Q.SHAPES, **ids)
def test_comparator_rejects_table_mutants(shape):
    H, W = shape
    tc = Q.table_case(H, W)
    t64, t32 = tc['tstats'][F64], tc['tstats'][F32]
    assert t64.shape == (3, 2, 3, H - 10, W - 10)
    assert R.ratio(t32, t64, t32) <= 1.0 <= Q.C['tmaps']
    rejected('tmaps', 'planes exchanged', t64.flip(1), t64, t32)
    for where in ('col', 'row'):
        rejected('tmaps', f'tap {where}', Q.tstats_ref(tc['frames'], F64, drop=where), t64, t32)
    cs = tc['frame'][2]
    for src, name in ((0, 'frame 0'), (1, 'frame 1')):
        terms = Q.with_struct(cs['ref'][F64], Q.struct_grad_from(cs['p'], cs['t'], t64[src, 0], t64[src, 1]))
        for loss in ('Fusion6', 'Fusion1'):
            rejected('dpred pixel', f'{name} {loss}', Q.combine(terms, loss), Q.dpred_ref(cs, loss, F64), Q.dpred_ref(cs, loss, F32))
    # the right frame's maps, handed in, give the reference
    own = Q.struct_grad_from(cs['p'], cs['t'], t64[2, 0], t64[2, 1])
    assert R.ratio(own, cs['ref'][F64]['struct'], cs['ref'][F32]['struct']) < 1e-3


def test_closed_forms():
    """loss_grad_ref and the scales against autograd, stats_from_partials against the loss itself"""
    cs = Q.case('tied', 3, 17, 65)
    for loss in ('L2', 'L1', 'Fusion7', 'Fusion8'):
        ref = Q.dpred_ref(cs, loss, F64, 4.0)
        got = Q.loss_grad_ref(cs['p'], cs['t'], loss, 4.0)
        assert float((got - ref.detach()).abs().max()) <= 2.0 ** -23 * float(ref.detach().abs().max())
    r = cs['ref'][F64]
    for loss in ('Fusion6', 'Fusion1', 'SSIM', 'Fusion7'):
        _, w1, w2, ws = Q.LOSSES[loss]
        st = Q.stats_from_partials(r['part_ssim'] if ws else None, r['part_l1'], loss, 3, 17, 65, 256.0)
        d = cs['p'].double() - cs['t'].double()
        want = 256.0 * (w1 * d.abs().mean() + w2 * (d * d).mean() + ws * (1 - r['map'].mean()))
        assert abs(st[0] - float(want)) <= 1e-7 * float(want) and abs(st[1] - float(d.abs().mean())) < 1e-12
