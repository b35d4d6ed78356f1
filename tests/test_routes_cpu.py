"""CPU: the kernel routes of a net (Net::settle_routes, read through mmvae_net_describe_routes) -- pinned for the shapes the project is built
around, checked against the rules between forward and backward over a sweep of configurations, and re-settled when the join-gradient form
is switched.  Host only: the net's constructor and its plan need no device."""
import ctypes
import importlib
import itertools

import pytest

F32, BF16, FP8 = 0, 1, 2                       # MMVAE_F32 / MMVAE_BF16 / MMVAE_FP8
ERR_UNSUPPORTED = -4                           # MMVAE_ERR_UNSUPPORTED
ENC_FIELDS = ["fwd_c1_cs_stream", "fwd_c2_stream", "bwd_pair_wgrad", "bwd_c2_late_reduce", "bwd_c2_dgrad_stream"]
DEC_FIELDS = ["fwd_cs_stream", "fwd_c2_stream", "fwd_stats_only", "fwd_join_conv1", "bwd_join_grad", "bwd_join_stream", "bwd_fuse_c2", "bwd_fuse_cs"]
NET_FIELDS = ["stem_fwd_stream", "stem_bwd_fused", "stem_dg_fused", "tail_fwd", "tail_bwd_fused", "tail_wg_in_reduce", "store8"]
# the messages of the rules settle_routes checks (csrc/vae_net.cpp)
RULES = ["fp8 storage of the last up-block needs the fused tail kernels", "fp8 storage of the last up-block needs tail_fwd_stream",
         "fp8 storage of the last up-block needs the fused tail backward", "fp8 storage of the last up-block needs join_bwd_stream",
         "the fused tail forward (no stored join) needs the fused tail backward", "the join-gradient form needs both fused passes"]


def _lib():
    return importlib.import_module("moving-mnist-vae_amd._lib").lib()


class _Net:
    def __init__(self, in_ch=1, z=128, out_ch=1, S=64, dtype=BF16, blocks=1):
        self.h = ctypes.c_void_p()
        assert _lib().mmvae_net_create_ex(ctypes.byref(self.h), in_ch, z, out_ch, S, 1, dtype, blocks) == 0, _lib().mmvae_last_error()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _lib().mmvae_net_destroy(self.h)

    def describe(self, N):
        """(0, text) or (error code, message)"""
        need = _lib().mmvae_net_describe_routes(self.h, N, None, 0)
        if need < 0:
            return need, _lib().mmvae_last_error().decode()
        buf = ctypes.create_string_buffer(need)
        assert _lib().mmvae_net_describe_routes(self.h, N, buf, need) == need
        short = ctypes.create_string_buffer(8)               # a short buffer is filled, terminated, and the length still reported
        assert _lib().mmvae_net_describe_routes(self.h, N, short, 8) == need and short.value == buf.value[:7]
        return 0, buf.value.decode()


def _parse(text):
    """[(name, {field: value})] in the printed order; every line must carry exactly its kind's fields, in order"""
    rows = []
    for line in text.strip().split("\n"):
        name, rest = line.split(": ")
        kv = [f.split("=") for f in rest.split(" ")]
        want = NET_FIELDS if name == "net" else ENC_FIELDS if name.startswith("encoder.") else DEC_FIELDS
        assert [k for k, _ in kv] == want, line
        rows.append((name, dict(kv)))
    assert rows[-1][0] == "net" and [n for n, _ in rows].count("net") == 1
    return rows


def _compact(rows):
    """name -> the fields that are set ("tail_fwd=X" as printed): the form the expectations below are written in"""
    return {name: " ".join(k if k != "tail_fwd" else "tail_fwd=" + v for k, v in f.items() if v != "0") for name, f in rows}


def _expect(nets, **lines):
    d = {n: "" for n in nets}
    d.update({k.replace("__", "."): v for k, v in lines.items()})
    return d


_ENC1 = ["encoder.layer%d.0" % i for i in range(1, 5)]
_ENC2 = ["encoder.layer%d.%d" % (i, b) for i in range(1, 5) for b in range(2)]
_DEC5 = ["decoder.uplayer%d.0" % i for i in range(1, 6)]
_L1 = "fwd_c1_cs_stream fwd_c2_stream bwd_pair_wgrad bwd_c2_late_reduce bwd_c2_dgrad_stream"
_UP4_JG = "fwd_c2_stream fwd_join_conv1 bwd_join_grad bwd_fuse_c2 bwd_fuse_cs"
_NET_BF16 = "stem_fwd_stream stem_bwd_fused stem_dg_fused tail_fwd=UP5 tail_bwd_fused tail_wg_in_reduce"
# (constructor arguments, expected routes); the same at N = 40 and N = 5120.  Confirmed when the record was introduced: with these fields the entry
# points launch, stream by stream, the kernel sequence they launched when each condition was evaluated in place (kernel traces of bf16, f32, deep
# and fp8), and three train steps of all seven nets end in the same bits.
PINNED = {
    "bf16": (dict(), _expect(
        _ENC1 + _DEC5 + ["net"], encoder__layer1__0=_L1, decoder__uplayer3__0="fwd_join_conv1", decoder__uplayer4__0=_UP4_JG,
        decoder__uplayer5__0="fwd_cs_stream fwd_c2_stream fwd_stats_only bwd_join_stream", net=_NET_BF16)),
    "f32": (dict(dtype=F32), _expect(_ENC1 + _DEC5 + ["net"], net="stem_bwd_fused tail_fwd=JOIN tail_bwd_fused tail_wg_in_reduce")),
    "deep": (dict(z=512, blocks=2), _expect(
        _ENC2 + ["decoder.uplayer%d.%d" % (i, b) for i in range(1, 6) for b in range(2)] + ["net"], encoder__layer1__0=_L1,
        encoder__layer1__1="fwd_c2_stream", decoder__uplayer4__1="fwd_c2_stream bwd_fuse_c2 bwd_fuse_cs",
        decoder__uplayer5__1="fwd_cs_stream fwd_c2_stream fwd_stats_only bwd_join_stream", net=_NET_BF16)),
    "fp8": (dict(dtype=FP8), _expect(
        _ENC1 + _DEC5 + ["net"], encoder__layer1__0=_L1, decoder__uplayer3__0="fwd_join_conv1", decoder__uplayer4__0=_UP4_JG,
        decoder__uplayer5__0="fwd_cs_stream fwd_c2_stream bwd_join_stream",
        net="stem_fwd_stream stem_bwd_fused stem_dg_fused tail_fwd=STREAM tail_bwd_fused tail_wg_in_reduce store8")),
    "S32": (dict(S=32), _expect(
        _ENC1 + _DEC5[:4] + ["net"], decoder__uplayer3__0="fwd_join_conv1", decoder__uplayer4__0="fwd_c2_stream bwd_fuse_c2 bwd_fuse_cs",
        net="stem_fwd_stream stem_bwd_fused tail_fwd=JOIN tail_bwd_fused tail_wg_in_reduce")),
    "out_ch3": (dict(out_ch=3), _expect(
        _ENC1 + _DEC5 + ["net"], encoder__layer1__0=_L1, decoder__uplayer3__0="fwd_join_conv1",
        decoder__uplayer4__0="fwd_c2_stream fwd_join_conv1 bwd_fuse_c2 bwd_fuse_cs", decoder__uplayer5__0="fwd_cs_stream fwd_c2_stream bwd_fuse_c2 bwd_fuse_cs",
        net="stem_fwd_stream stem_bwd_fused stem_dg_fused tail_fwd=GATHER tail_bwd_fused")),
    "in_ch3": (dict(in_ch=3), _expect(
        _ENC1 + _DEC5 + ["net"], encoder__layer1__0=_L1, decoder__uplayer3__0="fwd_join_conv1", decoder__uplayer4__0=_UP4_JG,
        decoder__uplayer5__0="fwd_cs_stream fwd_c2_stream fwd_stats_only bwd_join_stream", net="tail_fwd=UP5 tail_bwd_fused tail_wg_in_reduce")),
}


@pytest.mark.parametrize("N", [40, 5120])
@pytest.mark.parametrize("name", sorted(PINNED))
def test_routes_of_the_shapes_the_project_is_built_around(pkg, name, N):
    cfg, want = PINNED[name]
    with _Net(**cfg) as net:
        rc, text = net.describe(N)
    assert rc == 0, text
    got = _compact(_parse(text))
    assert list(got) == list(want), "blocks, in order"
    assert got == want, "\n" + text


def _check_rules(rows):
    """Every implication settle_routes guarantees, restated on the printed fields."""
    net = rows[-1][1]
    dec = [f for n, f in rows if n.startswith("decoder.")]
    enc = [f for n, f in rows if n.startswith("encoder.")]
    on = lambda f, k: f[k] == "1"                                                                      # noqa: E731
    last = dec[-1]
    # what the forward stored is what the backward reads
    if on(net, "store8"):                      # e4m3 y2 / ys of the last up-block: written and read only by the kernels that know the format
        assert net["tail_fwd"] == "STREAM" and on(net, "tail_wg_in_reduce") and on(last, "bwd_join_stream")
        assert on(last, "fwd_cs_stream") and on(last, "fwd_c2_stream")
    if net["tail_fwd"] != "GATHER":            # no stored join: the tail's weight gradient has to recompute it
        assert on(net, "tail_wg_in_reduce")
    assert on(net, "tail_wg_in_reduce") == (net["tail_fwd"] != "GATHER" and on(net, "tail_bwd_fused"))
    assert (net["tail_fwd"] == "UP5") == on(last, "fwd_stats_only")
    for i, f in enumerate(dec):
        if on(f, "bwd_join_grad"):             # the gradient arrives masked: the block above masks it, both consumers evaluate dy themselves
            assert on(f, "bwd_fuse_c2") and on(f, "bwd_fuse_cs")
            assert i + 1 < len(dec) and on(dec[i + 1], "bwd_join_stream")
        if on(f, "fwd_stats_only"):            # statistics-only launches exist for the stream kernel alone, and only the up5 tail stores for them
            assert on(f, "fwd_cs_stream") and on(f, "fwd_c2_stream") and i == len(dec) - 1
        if on(f, "bwd_join_stream"):           # the one-pass backward starts from the tail's gradient and leaves the fused passes nothing to do
            assert i == len(dec) - 1 and on(net, "tail_bwd_fused") and not on(f, "bwd_fuse_c2") and not on(f, "bwd_fuse_cs")
        if on(f, "fwd_join_conv1"):
            assert i + 1 < len(dec)
    if on(net, "stem_dg_fused"):               # the stem's backward recomputes layer1's data gradients: it is the fused stem pass
        assert on(net, "stem_bwd_fused")
    for i, f in enumerate(enc):
        if on(f, "bwd_c2_dgrad_stream") or on(f, "bwd_c2_late_reduce"):
            assert i == 0
        if on(f, "bwd_c2_dgrad_stream"):       # the flipped pack of conv2 (packs_enc_bwd) is the forward stream kernel's shape
            assert on(f, "fwd_c2_stream")


@pytest.mark.parametrize("S", [9, 16, 32, 33, 64])
@pytest.mark.parametrize("dtype", [F32, BF16, FP8])
def test_routes_fit_each_other_or_are_refused(pkg, dtype, S):
    for out_ch, blocks in itertools.product([1, 2, 3, 4, 8], [1, 2]):
        with _Net(out_ch=out_ch, S=S, dtype=dtype, blocks=blocks) as net:
            for N in (1, 40, 5120):
                rc, text = net.describe(N)
                if rc != 0:
                    assert rc == ERR_UNSUPPORTED and any(r in text for r in RULES), (out_ch, blocks, N, rc, text)
                    continue
                rows = _parse(text)
                assert len(rows) == 1 + 4 * blocks + (5 if S > 32 else 4) * blocks, (out_ch, blocks, N)
                _check_rules(rows)


def test_switching_the_join_gradient_form_settles_the_routes_again(pkg):
    with _Net() as net:
        rc, default = net.describe(40)
        assert rc == 0 and any(f["bwd_join_grad"] == "1" for n, f in _parse(default) if n.startswith("decoder."))
        assert _lib().mmvae_net_set_join_grad(net.h, 0) == 0
        rc, off = net.describe(40)
        assert rc == 0 and all(f["bwd_join_grad"] == "0" for n, f in _parse(off) if n.startswith("decoder."))
        _check_rules(_parse(off))
        assert off == default.replace("bwd_join_grad=1", "bwd_join_grad=0"), "nothing else moves"
        assert _lib().mmvae_net_set_join_grad(net.h, 1) == 0
        assert net.describe(40) == (0, default)


def test_describe_routes_rejects_bad_arguments(pkg):
    with _Net() as net:
        assert _lib().mmvae_net_describe_routes(None, 40, None, 0) < 0
        assert _lib().mmvae_net_describe_routes(net.h, 0, None, 0) < 0
        assert _lib().mmvae_net_describe_routes(net.h, 40, None, 16) < 0
