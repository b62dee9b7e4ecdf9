"""CPU: the host side of the wide fused block -- the branch-aligned grouping of the depthwise stage (cat_amd/fused_unit.py dw_launches), the
per-launch filter frames a plan's preparation jobs write, and the register budget of the statistics-writing wide stage-1 kernel
(csrc/conv_s1ws.hip), which keeps two workgroups per CU like the kernel it shares its main loop with."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _covers(quads, spans):
    """the spans are consecutive, in order, and together every branch exactly once (no branch split: a span is a range of whole branches)"""
    assert spans[0][0] == 0 and spans[-1][1] == len(quads)
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and all(b0 < b1 for b0, b1 in spans)


def test_depthwise_launch_grouping():
    from cat_amd import _lib as L, fused_unit as U
    assert L.DWM_MAXQ_BWD == 18 and L.DWM_MAXQ == 24
    groups = lambda quads, maxq=L.DWM_MAXQ_BWD: U.dw_launches(quads, maxq)
    assert groups([11, 11, 11]) == [(0, 1), (1, 2), (2, 3)]      # the teacher: 11 | 11 | 11
    assert groups([7, 7, 7]) == [(0, 2), (2, 3)]                 # ngf 40: 14 | 7
    assert groups([18]) == [(0, 1)] and groups([6, 6, 6]) == [(0, 3)] and groups([4, 5, 0]) == [(0, 3)]      # up to 18 quads: one launch, as before
    assert groups([19]) is None and groups([3, 19, 2]) is None   # a single branch wider than a launch
    assert groups([]) == []
    assert groups([11, 11, 11], L.DWM_MAXQ) == [(0, 2), (2, 3)]  # the forward-only frozen teacher keeps 22 + 11
    for quads in ([11, 11, 11], [7, 7, 7], [18, 18, 1], [1, 17, 1, 17, 2], [9, 9, 9, 9, 9], [12, 6, 13, 5]):
        spans = groups(quads)
        _covers(quads, spans)
        assert all(sum(quads[b0:b1]) <= L.DWM_MAXQ_BWD for b0, b1 in spans)
        # greedy: the next branch did not fit into the launch before it
        assert all(sum(quads[b0:b1]) + quads[b1] > L.DWM_MAXQ_BWD for b0, b1 in spans[:-1])


def test_frozen_teacher_grouping_is_the_same_function():
    from cat_amd import frozen_in, fused_unit as U, _lib as L
    for quads in ([11, 11, 11], [8, 8, 8], [24, 1, 23], [25], []):
        assert frozen_in.dw_launches(quads) == U.dw_launches(quads, L.DWM_MAXQ)


def test_wide_stage1_kernel_keeps_two_workgroups_per_cu():
    import codegen_table
    t = codegen_table.table('cat_amd/csrc/conv_s1ws.hip')
    hit = {k: v for k, v in t.items() if 'tstage1ws_kernel' in k}
    assert len(hit) == 1, sorted(t)
    for k, v in hit.items():
        assert v['vgpr'] <= 256 and v['scratch'] == 0 and v['vspill'] == 0, (k, v)


def test_switch_names():
    from cat_amd import fused_block, fused_unit
    old = fused_block.set_wide(False)
    assert fused_block.set_wide(old) is False
    old = fused_unit.set_stage1_wide(False)
    assert fused_unit.set_stage1_wide(old) is False
