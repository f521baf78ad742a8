"""The guard helper of the tail tests (tests/_guards.py) on CPU tensors: it must flag a write into a guard, a canary left in an
output and a one-bit difference between placements -- otherwise the GPU tests that rely on it could pass vacuously."""
import pytest
import torch

from _guards import Guards, assert_same_outputs, is_canary, run_both

DTYPES = [torch.float32, torch.float16, torch.float64, torch.int32, torch.uint8]


def _data(dtype, n):
    return (torch.arange(n) % 7 + 1).to(dtype)


@pytest.mark.parametrize("minimal", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_placement_alignment_and_clean_call_passes(dtype, minimal):
    es = torch.empty((), dtype=dtype).element_size()
    for align in sorted({es, 4 if es <= 4 else es, 8, 16}):
        g = Guards("cpu", minimal)
        x = g.inp(_data(dtype, 37), align)
        y = g.out((37,), dtype, align)
        assert x.data_ptr() % align == 0 and y.data_ptr() % align == 0
        if minimal:
            assert x.data_ptr() % (2 * align) != 0 and y.data_ptr() % (2 * align) != 0
        else:
            assert x.data_ptr() % 256 == 0
        assert torch.equal(x, _data(dtype, 37)) and bool(is_canary(y).all())
        y.copy_(x)
        g.check()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["front", "back"])
@pytest.mark.parametrize("kind", ["inp", "out", "io"])
def test_planted_guard_write_is_flagged(dtype, where, kind):
    g = Guards("cpu", minimal=True)
    t = g.out((33,), dtype, 8) if kind == "out" else getattr(g, kind)(_data(dtype, 33), 8)
    if kind == "out":
        t.copy_(_data(dtype, 33))
    p = g.placed[0]
    k = p.lo - 1 if where == "front" else p.lo + p.nbytes   # the byte just before / just after the buffer
    p.buf[k] ^= 1
    with pytest.raises(AssertionError, match="guard changed"):
        g.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_canary_in_output_is_flagged(dtype):
    g = Guards("cpu")
    y = g.out((40,), dtype, 4 if dtype != torch.float64 else 8)
    y.copy_(_data(dtype, 40))
    g.check()
    y[39] = torch.tensor(0, dtype=dtype)
    y.view(torch.uint8)[-y.element_size():].copy_(g.placed[0].buf[:y.element_size()])   # row n - 1 left at the canary
    with pytest.raises(AssertionError, match="still hold the canary"):
        g.check()


def test_written_and_untouched_masks():
    g = Guards("cpu")
    y = g.out((4, 3), torch.float32, 4, written=torch.tensor([True, False, True, False])[:, None],
              untouched=torch.tensor([False, True, False, True])[:, None])
    y[0] = 1.0
    y[2] = 2.0
    g.check()
    y[3, 1] = 0.0   # a row the contract leaves alone
    with pytest.raises(AssertionError, match="leaves alone"):
        g.check()


def test_one_bit_difference_between_placements_is_flagged():
    def call(g, flip):
        x = g.inp(torch.linspace(-1, 1, 50), 4)
        y = g.out((50,), torch.float32, 4)
        y.copy_(x * 3)
        if flip and g.minimal:
            y.view(torch.int32)[17] ^= 1
        return y
    run_both("cpu", lambda g: call(g, False))
    with pytest.raises(AssertionError, match="differs between"):
        run_both("cpu", lambda g: call(g, True))
    a = [torch.zeros(8, dtype=torch.uint8)]
    b = [a[0].clone()]
    b[0][3] = 0x80
    with pytest.raises(AssertionError):
        assert_same_outputs(a, b)


def test_input_guards_are_poison():
    g = Guards("cpu", minimal=True)
    g.inp(torch.ones(5), 4)
    g.inp(torch.ones(5, dtype=torch.float16), 2)
    g.inp(torch.ones(5, dtype=torch.int32), 4)
    g.inp(torch.ones(5, dtype=torch.uint8), 1)
    f32, f16, i32, u8 = g.placed
    assert bool(torch.isnan(f32.buf[:f32.lo].view(torch.float32)).all())
    assert bool(torch.isnan(f16.buf[:f16.lo].view(torch.float16)).all())
    assert bool((i32.buf[:i32.lo].view(torch.int32) == 2 ** 31 - 1).all())
    assert set(u8.buf[:u8.lo].tolist()) == {0x01, 0xFF}
    # and no poison is mistaken for the canary
    assert not bool(is_canary(f32.buf[:f32.lo].view(torch.float32)).any())
