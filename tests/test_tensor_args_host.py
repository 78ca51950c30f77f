"""The layout rules of the device-tensor entry points (mod16_amd/_tensors.py) on CPU tensors: the
helpers look at shape and stride() only, so views built with as_strided and slicing exercise every
edge without a GPU. What is asserted is what mod16_amd.raster has always applied to its tensors: unit
stride in the last dimension unless it has at most one element, rows at least a row apart (one row:
its length, whatever its stride), planes at least a plane apart (one plane: exactly a plane)."""
import numpy as np
import pytest
import torch

from mod16_amd import _tensors as T


def strided(shape, stride):
    """A float32 CPU tensor of that shape and those strides (elements), over storage large enough."""
    need = 1 + sum((n - 1) * s for n, s in zip(shape, stride) if n > 0)
    return torch.zeros(max(need, 1)).as_strided(shape, stride)


# ------------------------------------------------------------------ rows
def test_row_pitch_of_dense_and_pitched_rows():
    assert T.row_pitch(torch.zeros(3, 7), 'x') == 7
    assert T.row_pitch(torch.zeros(3, 12)[:, :7], 'x') == 12
    assert T.row_pitch(torch.zeros(4, 3, 12)[1:, :, 2:9], 'x') == 12       # the last two dimensions count
    assert T.row_pitch(torch.zeros(7), 'x') == 7                            # (n,): one row


@pytest.mark.parametrize('stride', [0, 1, 3, 7, 100])
def test_one_row_reports_its_length_whatever_its_stride(stride):
    assert T.row_pitch(strided((1, 7), (stride, 1)), 'x') == 7


def test_rows_of_length_0_and_1_have_no_inner_stride_to_check():
    assert T.row_pitch(strided((3, 1), (5, 9)), 'x') == 5
    assert T.row_pitch(strided((3, 0), (5, 9)), 'x') == 5
    assert T.row_pitch(strided((1, 1), (0, 9)), 'x') == 1
    assert T.row_pitch(strided((1, 0), (0, 9)), 'x') == 1                   # never 0: a pitch is at least 1
    assert T.row_pitch(strided((1,), (4,)), 'x') == 1
    assert T.row_pitch(strided((3, 0), (0, 1)), 'x') == 0                   # several empty rows: their stride


def test_pitch_of_exactly_a_row_passes_and_one_below_is_refused():
    assert T.row_pitch(strided((3, 7), (7, 1)), 'x') == 7
    with pytest.raises(ValueError, match=r'^x: the distance between rows must be at least 7$'):
        T.row_pitch(strided((3, 7), (6, 1)), 'x')
    with pytest.raises(ValueError, match=r'^qc: the stride in time must be at least 7$'):
        T.row_pitch(torch.zeros(1, 7).expand(3, 7), 'qc', 'stride in time')


def test_non_unit_inner_stride_is_refused():
    with pytest.raises(ValueError, match=r'^x must have unit stride in pixels$'):
        T.row_pitch(torch.zeros(3, 14)[:, ::2], 'x')
    with pytest.raises(ValueError, match='unit stride'):
        T.row_pitch(torch.zeros(14)[::2], 'x')
    with pytest.raises(ValueError, match='unit stride'):
        T.row_pitch(torch.zeros(7, 3).t(), 'x')


# ---------------------------------------------------------------- planes
def test_plane_layout_of_dense_and_pitched_planes():
    assert T.plane_layout(torch.zeros(4, 3, 5), 'x') == (5, 15)
    assert T.plane_layout(torch.zeros(4, 4, 8)[:, :3, :5], 'x') == (8, 32)
    assert T.plane_layout(torch.zeros(3, 5), 'x') == (5, 15)
    assert T.plane_layout(torch.zeros(4, 8)[:3, 1:6], 'x') == (8, 21)


@pytest.mark.parametrize('stride', [0, 1, 16, 1000])
def test_one_plane_reports_exactly_a_plane(stride):
    assert T.plane_layout(strided((1, 3, 5), (stride, 8, 1)), 'x') == (8, 2 * 8 + 5)
    assert T.plane_layout(strided((3, 5), (8, 1)), 'x') == (8, 2 * 8 + 5)


@pytest.mark.parametrize('stride', [0, 1, 3, 100])
def test_one_row_of_a_plane_reports_the_row_length(stride):
    assert T.plane_layout(strided((2, 1, 5), (9, stride, 1)), 'x') == (5, 9)
    assert T.plane_layout(strided((1, 5), (stride, 1)), 'x') == (5, 5)


def test_columns_of_length_0_and_1_have_no_inner_stride_to_check():
    assert T.plane_layout(strided((2, 3, 1), (40, 4, 9)), 'x') == (4, 40)
    assert T.plane_layout(strided((2, 3, 0), (40, 4, 9)), 'x') == (4, 40)
    assert T.plane_layout(strided((1, 0), (7, 9)), 'x') == (0, 0)           # one empty row: its length


def test_plane_pitch_of_exactly_a_row_passes_and_one_below_is_refused():
    assert T.plane_layout(strided((2, 3, 5), (15, 5, 1)), 'x') == (5, 15)
    with pytest.raises(ValueError, match=r'^x: the distance between rows must be at least 5$'):
        T.plane_layout(strided((2, 3, 5), (15, 4, 1)), 'x')
    with pytest.raises(ValueError, match='distance between rows'):
        T.plane_layout(torch.zeros(1, 5).expand(3, 5), 'x')


def test_plane_stride_of_exactly_a_plane_passes_and_one_below_is_refused():
    assert T.plane_layout(strided((2, 3, 5), (21, 8, 1)), 'x') == (8, 21)
    with pytest.raises(ValueError, match=r'^x: the stride in time must be at least a plane \(21 elements\)$'):
        T.plane_layout(strided((2, 3, 5), (20, 8, 1)), 'x')
    with pytest.raises(ValueError, match='stride in time'):
        T.plane_layout(torch.zeros(1, 3, 5).expand(4, 3, 5), 'x')


def test_non_unit_column_stride_is_refused():
    with pytest.raises(ValueError, match=r'^x must have unit stride in columns$'):
        T.plane_layout(torch.zeros(2, 3, 10)[:, :, ::2], 'x')
    with pytest.raises(ValueError, match='unit stride'):
        T.plane_layout(torch.zeros(5, 3).t(), 'x')


# ------------------------------------------------------ sharing, devices
def test_share_one():
    assert T.share_one([12, 12, 12], 'the fields', 'pitch') == 12
    assert T.share_one([(8, 21), (8, 21)], 'the fields', 'pitch') == (8, 21)
    assert T.share_one([], 'the fields', 'pitch') is None
    with pytest.raises(ValueError, match=r'^the fields must share one distance between rows$'):
        T.share_one([12, 13], 'the fields', 'distance between rows')


def test_a_cpu_tensor_and_a_non_tensor_are_refused_with_type_error():
    with pytest.raises(TypeError, match=r'^x must be a float32 tensor on cuda:0$'):
        T.check_device(torch.zeros(3), 'x', 0, torch.float32)
    with pytest.raises(TypeError, match=r'^x must be a uint8 or int32 tensor on cuda:1$'):
        T.check_device(torch.zeros(3, dtype=torch.uint8), 'x', 1, torch.uint8, torch.int32)
    with pytest.raises(TypeError, match=r'^x must be a tensor on cuda:0$'):
        T.check_device(torch.zeros(3), 'x', 0)
    for other in (None, 1.0, [1.0, 2.0]):
        with pytest.raises(TypeError, match='tensor on cuda:0'):
            T.check_device(other, 'x', 0, torch.float32)
    with pytest.raises(TypeError, match='tensor on cuda:0'):                 # the device test comes first
        T.series(torch.zeros(2, 7, dtype=torch.float64), 'x', 7, 0, torch.float64)


# ------------------------------------------------------- the out= protocol
def test_numpy_and_torch_dtypes_map_both_ways():
    for name in ('float32', 'float64', 'uint8', 'uint16', 'int32', 'int64'):
        assert T.torch_dtype(name) is getattr(torch, name) and T.torch_dtype(np.dtype(name)) is getattr(torch, name)
        assert T.numpy_dtype(getattr(torch, name)) == np.dtype(name)


@pytest.fixture
def on_cpu(monkeypatch):
    """named_outputs on CPU tensors: the device test is replaced by one of the dtype alone, and what is
    allocated lands on the CPU. -> the labels in the order in which they were checked"""
    seen = []

    def check_device(t, what, device, *dtypes):
        seen.append(what)
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
            raise TypeError('%s must be a tensor on cuda:%d' % (what, device))
    monkeypatch.setattr(T, 'check_device', check_device)
    monkeypatch.setattr(torch, 'device', lambda kind, index: 'cpu')
    return seen


NAMED = {'z': ((3, 7), np.dtype(np.float32)), 'count': ((2, 7), np.dtype(np.uint8))}
PLANES = {'mean': ((2, 3, 5), np.dtype(np.float64)), 'annual': ((3, 5), np.dtype(np.float64))}
NUMBERED = {0: ((3, 7), np.dtype(np.float64)), 1: ((3, 7), np.dtype(np.uint16))}


def test_named_outputs_allocates_what_the_table_states(on_cpu):
    outs, lay = T.named_outputs(None, NAMED, 0, 'stride in time')
    assert list(outs) == ['z', 'count'] and lay == {'z': 7, 'count': 7}
    assert [(tuple(t.shape), t.dtype) for t in outs.values()] == [((3, 7), torch.float32), ((2, 7), torch.uint8)]
    outs, lay = T.named_outputs(None, PLANES, 0)
    assert lay == {'mean': (5, 15), 'annual': (5, 15)} and outs['annual'].shape == (3, 5)
    outs, lay = T.named_outputs(None, NUMBERED, 0, 'distance between rows')
    assert list(outs) == [0, 1] and outs[1].dtype == torch.uint16 and lay == {0: 7, 1: 7}
    assert on_cpu == ["out['z']", "out['count']", "out['mean']", "out['annual']", 'out[0]', 'out[1]']


def test_named_outputs_takes_the_callers_tensors_in_the_tables_order(on_cpu):
    z, count = torch.zeros(3, 12)[:, 2:9], torch.zeros(2, 7, dtype=torch.uint8)
    outs, lay = T.named_outputs({'count': count, 'z': z}, NAMED, 0, 'stride in time')
    assert list(outs) == ['z', 'count'] and outs['z'] is z and outs['count'] is count
    assert lay == {'z': 12, 'count': 7}
    mean, annual = torch.zeros(2, 4, 8, dtype=torch.float64)[:, :3, :5], torch.zeros(3, 5, dtype=torch.float64)
    outs, lay = T.named_outputs(dict(mean=mean, annual=annual), PLANES, 0)
    assert lay == {'mean': (8, 32), 'annual': (5, 15)}
    a, b = torch.zeros(3, 7, dtype=torch.float64), torch.zeros(3, 9, dtype=torch.uint16)[:, :7]
    for out in ([a, b], (a, b), iter([a, b])):
        outs, lay = T.named_outputs(out, NUMBERED, 0, 'distance between rows')
        assert outs[0] is a and outs[1] is b and lay == {0: 7, 1: 9}


def test_named_outputs_refuses_another_key_set_or_count_before_it_looks_at_a_tensor(on_cpu):
    z, count = torch.zeros(3, 7), torch.zeros(2, 7, dtype=torch.uint8)
    for out in ({'z': z}, {'z': z, 'count': count, 'pct': z}, {'z': z, 'pct': count}, {}):
        with pytest.raises(ValueError, match=r'^out must hold exactly the fields produced: z, count$'):
            T.named_outputs(out, NAMED, 0, 'stride in time')
    with pytest.raises(ValueError, match=r'^out must hold exactly the requested outputs: z, count$'):
        T.named_outputs({'z': None}, NAMED, 0, 'stride in time', called='requested outputs')
    for out in ([z], [z, z, z], []):
        with pytest.raises(ValueError, match=r'^out must hold 2 tensors$'):
            T.named_outputs(out, NUMBERED, 0, 'distance between rows')
    assert on_cpu == []


def test_named_outputs_checks_device_then_shape_then_layout_result_by_result(on_cpu):
    good = torch.zeros(3, 7)
    count = torch.zeros(2, 7, dtype=torch.uint8)
    with pytest.raises(TypeError, match=r"^out\['z'\] must be a tensor on cuda:0$"):     # wrong in every way: the type
        T.named_outputs(dict(z=torch.zeros(3, 6, dtype=torch.int16)[:, ::2], count=count), NAMED, 0, 'stride in time')
    with pytest.raises(ValueError, match=r"^out\['z'\] must have shape \(3, 7\), got \(3, 3\)$"):      # shape before layout
        T.named_outputs(dict(z=torch.zeros(3, 6)[:, ::2], count=count), NAMED, 0, 'stride in time')
    with pytest.raises(ValueError, match=r"^out\['z'\] must have unit stride in pixels$"):
        T.named_outputs(dict(z=torch.zeros(3, 14)[:, ::2], count=count), NAMED, 0, 'stride in time')
    with pytest.raises(ValueError, match=r"^out\['z'\]: the stride in time must be at least 7$"):
        T.named_outputs(dict(z=torch.zeros(1, 7).expand(3, 7), count=count), NAMED, 0, 'stride in time')
    with pytest.raises(ValueError, match=r"^out\['mean'\]: the stride in time must be at least a plane \(15 elements\)$"):
        T.named_outputs(dict(mean=torch.zeros(1, 3, 5, dtype=torch.float64).expand(2, 3, 5),
                             annual=torch.zeros(3, 5, dtype=torch.float64)), PLANES, 0)
    # two offences in different results: the earlier result's, whatever its kind
    del on_cpu[:]
    with pytest.raises(ValueError, match=r"^out\['z'\] must have unit stride in pixels$"):
        T.named_outputs(dict(z=torch.zeros(3, 14)[:, ::2], count=good), NAMED, 0, 'stride in time')
    assert on_cpu == ["out['z']"]
    with pytest.raises(TypeError, match=r'^out\[1\] must be a tensor on cuda:0$'):
        T.named_outputs([torch.zeros(3, 7, dtype=torch.float64), good], NUMBERED, 0, 'distance between rows')
    with pytest.raises(ValueError, match=r'^out\[0\] must have shape \(3, 7\), got \(3, 6\)$'):
        T.named_outputs([torch.zeros(3, 6, dtype=torch.float64), good], NUMBERED, 0, 'distance between rows')
