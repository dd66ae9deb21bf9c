"""The bf16 row kernels of csrc/encoder_ops.hip (k_add_layernorm, k_embed_layernorm, k_final_layernorm, k_bias_layernorm) through
their four entry points against the fp64 reference of tests/layernorm_cases.py, elementwise inside its derived bound
(2^-8 |ref| + c 2^-24 (max_row|v| rstd |gamma| + |beta|)): every width 256 .. 2048, row counts around the four rows a wavefront
of k_bias_layernorm takes and around a workgroup's last wavefronts, the row arithmetic of skip, T and registers at its edges, both
output types, rows of mean 30, of magnitude 1e-3 (eps decides), constant rows and gamma near 0.  xout is bit-exact, the f32 output
is the bf16 one widened, 64 sentinel rows around every output stay untouched, the inputs stay as they were, and rejected arguments
write nothing."""
import ctypes as C
import zlib

import pytest

import layernorm_cases as LC

pytestmark = pytest.mark.gpu

GUARD = 64
BSC_E_INVALID = -1


def seed_of(*a):
    return zlib.crc32(" ".join(map(str, a)).encode())


def lib():
    from bsc_nav_amd import _lib
    return _lib.load()


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def guarded(rows, width, f32=False):
    """an output of `rows` rows with GUARD sentinel rows on either side"""
    import torch
    if f32:
        return torch.full((rows + 2 * GUARD, width), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    return torch.full((rows + 2 * GUARD, width), 0x5A5A, dtype=torch.int16, device="cuda")


def inner(buf):
    return buf[GUARD:]


def guards_intact(buf):
    s = 0x5A5A5A5A if buf.element_size() == 4 else 0x5A5A
    return bool((buf[:GUARD] == s).all()) and bool((buf[-GUARD:] == s).all())


def untouched(buf):
    return bool((buf == (0x5A5A5A5A if buf.element_size() == 4 else 0x5A5A)).all())


def values(buf):
    """the rows between the guards as f32"""
    import torch
    body = buf[GUARD:-GUARD]
    return body.view(torch.float32) if buf.dtype == torch.int32 else body.view(torch.bfloat16).float()


def on_gpu(z):
    """the case's tensors as the kernels read them: bf16 (exact, they are bf16 numbers), bias_sum f32"""
    import torch
    return {k: (v.cuda() if k == "bias_sum" else v.cuda().bfloat16()).contiguous() for k, v in z.items()}


def inside(tag, y, ref, bound, worst):
    r = LC.worst_ratio(y, ref, bound)
    worst[0] = max(worst[0], r)
    assert r <= 1.0, (tag, r)


@pytest.mark.parametrize("width", LC.WIDTHS)
def test_add_layernorm(width):
    import torch
    for family in LC.FAMILIES:
        worst = [0.0]
        for rows in LC.ADD_ROWS:
            z = LC.make("add", family, rows, width, seed_of("add", family, rows, width), device="cuda")
            d = on_gpu(z)
            keep = {k: t.clone() for k, t in d.items()}
            for with_delta in (True, False):
                v = LC.rows_add(z, with_delta)
                ref, bound = LC.layernorm64(v, z["gamma"], z["beta"])
                y, xout = guarded(rows, width), guarded(rows, width)
                st = lib().bsc_enc_add_layernorm(ptr(d["x"]), ptr(d["delta"]) if with_delta else None, ptr(d["gamma"]), ptr(d["beta"]),
                                                 ptr(inner(xout)), ptr(inner(y)), rows, width, LC.EPS, stream())
                torch.cuda.synchronize()
                assert st == 0 and guards_intact(y) and guards_intact(xout), (family, rows, with_delta, st)
                inside(("add", family, rows, with_delta), values(y), ref, bound, worst)
                if with_delta:
                    assert torch.equal(values(xout), v), (family, rows, "xout is not bf16(x + delta)")
                else:
                    assert untouched(xout)
            assert all(torch.equal(d[k], keep[k]) for k in d)
        print(f"rows k_add_layernorm width {width} {family}: worst |y - ref| / bound = {worst[0]:.3f}")


@pytest.mark.parametrize("width", LC.WIDTHS)
def test_embed_layernorm(width):
    import torch
    for family in LC.FAMILIES:
        worst = [0.0]
        for shape in LC.EMBED_SHAPES:
            B, T, R = shape
            z = LC.make("embed", family, shape, width, seed_of("embed", family, shape, width), device="cuda")
            d = on_gpu(z)
            keep = {k: t.clone() for k, t in d.items()}
            v = LC.rows_embed(z, shape)
            ref, bound = LC.layernorm64(v, z["gamma"], z["beta"])
            y, xout = guarded(B * T, width), guarded(B * T, width)
            st = lib().bsc_enc_embed_layernorm(ptr(d["patch"]), ptr(d["cls"]), ptr(d["reg"]) if R else None, ptr(d["pos"]), ptr(d["gamma"]),
                                               ptr(d["beta"]), ptr(inner(xout)), ptr(inner(y)), B, T, R, width, LC.EPS, stream())
            torch.cuda.synchronize()
            assert st == 0 and guards_intact(y) and guards_intact(xout), (family, shape, st)
            assert torch.equal(values(xout), v), (family, shape, "xout is not the assembled token rows")
            inside(("embed", family, shape), values(y), ref, bound, worst)
            assert all(torch.equal(d[k], keep[k]) for k in d)
        print(f"rows k_embed_layernorm width {width} {family}: worst |y - ref| / bound = {worst[0]:.3f}")


@pytest.mark.parametrize("width", LC.WIDTHS)
@pytest.mark.parametrize("op", ["final", "bias"])
def test_final_and_bias_layernorm(op, width):
    import torch
    for family in LC.FAMILIES:
        worst = [0.0]
        for shape in (LC.FINAL_SHAPES if op == "final" else LC.BIAS_SHAPES):
            B, T, skip = shape
            n = B * (T - skip)
            z = LC.make(op, family, shape, width, seed_of(op, family, shape, width), device="cuda")
            d = on_gpu(z)
            keep = {k: t.clone() for k, t in d.items()}
            v = LC.rows_final(z, shape) if op == "final" else LC.rows_bias(z, shape)
            ref, bound = LC.layernorm64(v, z["gamma"], z["beta"])
            got = {}
            for f32 in (0, 1):
                y = guarded(n, width, bool(f32))
                if op == "final":
                    st = lib().bsc_enc_final_layernorm(ptr(d["x"]), ptr(d["delta"]), ptr(d["gamma"]), ptr(d["beta"]), ptr(inner(y)), f32,
                                                       B, T, skip, width, LC.EPS, stream())
                else:
                    st = lib().bsc_enc_bias_layernorm(ptr(d["u"]), ptr(d["bias_sum"]), ptr(d["gamma"]), ptr(d["beta"]), ptr(inner(y)), f32,
                                                      B, T, skip, width, LC.EPS, stream())
                torch.cuda.synchronize()
                assert st == 0 and guards_intact(y), (op, family, shape, f32, st)
                got[f32] = values(y)
                inside((op, family, shape, f32), got[f32], ref, bound, worst)
            assert torch.equal(got[0], got[1]), (op, family, shape, "the f32 output is not the bf16 one widened")
            assert all(torch.equal(d[k], keep[k]) for k in d), (op, family, shape, "an input changed")
        print(f"rows k_{op}_layernorm width {width} {family}: worst |y - ref| / bound = {worst[0]:.3f}")


class Refusals:
    """Well-formed arguments of the four entry points for one (width, B, T, R, skip); call(entry, name=value, ...) replaces the
    named ones and returns the status.  The outputs are guarded buffers that a refused call must leave all-sentinel."""
    ORDER = {"add": ("x", "delta", "gamma", "beta", "xout", "y", "rows", "width", "eps"),
             "embed": ("patch", "cls", "reg", "pos", "gamma", "beta", "xout", "y", "B", "T", "R", "width", "eps"),
             "final": ("x", "delta", "gamma", "beta", "y", "f32", "B", "T", "skip", "width", "eps"),
             "bias": ("x", "bias", "gamma", "beta", "y", "f32", "B", "T", "skip", "width", "eps")}

    def __init__(self, width, B, T, R, skip):
        import torch
        rows = B * T
        t = lambda n: torch.zeros((max(n, 1), width), dtype=torch.bfloat16, device="cuda")
        self.keep = [t(rows), t(rows), t(1), t(1), t(1), t(R), t(T), t(rows), torch.zeros(width, dtype=torch.float32, device="cuda")]
        x, delta, gamma, beta, cls, reg, pos, patch, bias = self.keep
        self.y, self.xout, self.y32 = guarded(rows, width), guarded(rows, width), guarded(rows, width, True)
        self.args = dict(x=ptr(x), delta=ptr(delta), gamma=ptr(gamma), beta=ptr(beta), cls=ptr(cls), reg=ptr(reg), pos=ptr(pos),
                         patch=ptr(patch), bias=ptr(bias), xout=ptr(inner(self.xout)), y=ptr(inner(self.y)), rows=rows, width=width,
                         eps=LC.EPS, B=B, T=T, R=R, skip=skip, f32=0)

    def call(self, entry, **replace):
        a = dict(self.args)
        a.update(replace)
        if a["f32"] and "y" not in replace:
            a["y"] = ptr(inner(self.y32))
        fn = getattr(lib(), f"bsc_enc_{entry}_layernorm")
        return fn(*[a[k] for k in self.ORDER[entry]], stream())

    def nothing_written(self):
        import torch
        torch.cuda.synchronize()
        return untouched(self.y) and untouched(self.xout) and untouched(self.y32)


def test_rejected_arguments_write_nothing():
    two_outputs = [(e, f32) for e in ("final", "bias") for f32 in (0, 1)]
    cases = []                                          # (what, Refusals, statuses)
    for width in (192, 2304):
        r = Refusals(width, 2, 6, 4, 1)
        cases.append((f"width {width}", r, [r.call("add"), r.call("embed")] + [r.call(e, f32=f) for e, f in two_outputs]))
    for skip in (6, 7):
        r = Refusals(256, 2, 6, 4, skip)
        cases.append((f"T = 6 <= skip = {skip}", r, [r.call(e, f32=f) for e, f in two_outputs]))
    r = Refusals(256, 2, 5, 4, 1)
    cases.append(("T = 5 < 2 + registers = 6", r, [r.call("embed")]))
    r = Refusals(256, 2, 6, 4, 1)
    cases.append(("registers without reg", r, [r.call("embed", reg=None)]))
    cases.append(("delta without xout", r, [r.call("add", xout=None)]))
    cases.append(("no rows", r, [r.call("add", rows=0), r.call("add", rows=-1), r.call("embed", B=0)] +
                  [r.call(e, f32=f, B=0) for e, f in two_outputs]))
    null = [r.call("add", **{k: None}) for k in ("x", "gamma", "beta", "y")]
    null += [r.call("embed", **{k: None}) for k in ("patch", "cls", "pos", "gamma", "beta", "xout", "y")]
    null += [r.call("final", **{k: None}) for k in ("x", "delta", "gamma", "beta", "y")]
    null += [r.call("bias", **{k: None}) for k in ("x", "bias", "gamma", "beta", "y")]
    cases.append(("null pointer", r, null))
    for what, r, statuses in cases:
        assert statuses and all(st == BSC_E_INVALID for st in statuses), (what, statuses)
        assert r.nothing_written(), what
    # the same arguments unreplaced are served, so it is the replaced one that each call above was refused for
    ok = [r.call("add"), r.call("embed")] + [r.call(e, f32=f) for e, f in two_outputs]
    assert all(st == 0 for st in ok), ok
    assert not r.nothing_written() and guards_intact(r.y) and guards_intact(r.xout) and guards_intact(r.y32)
