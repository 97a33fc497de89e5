"""The host-side plans of the convolution kernels, pinned: ffwm_conv3x3_winograd_splits, ffwm_conv3x3_winograd_workspace_bytes and
ffwm_conv2d_forward_workspace launch nothing, so they answer without a GPU (the library then counts 256 compute units, the
MI355X's number).  Python routes on these answers (conv.py: Winograd or not; flownet_eval.py: the split workspace), and the launches
read the same plan functions, so a changed answer is a changed launch.

The expected values are literals.  They were produced by the library of the commit BEFORE the one that introduced WinoPlan (the
three Winograd entry points then derived their route separately), never by the code under test."""
import pytest


@pytest.fixture(scope="module")
def hiplib():
    from ffwm_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.fixture
def options(hiplib):
    """set(name, value) for the test; every option it touched gets its previous value back."""
    prev = []

    def set_option(name, value):
        old = hiplib.ffwm_set_option(name.encode(), value)
        assert old >= 0, name
        prev.append((name, old))

    yield set_option
    for name, old in reversed(prev):
        hiplib.ffwm_set_option(name.encode(), old)


# ({option: value}, (B, C, H, W, K, act), splits)
WINO_SPLITS = [
    # not raw-staged: width, odd height, tile rows that do not fill whole workgroups (TH % (64 / TW) != 0)
    ({}, (1, 8, 10, 12, 64, 0), 1),
    ({}, (1, 512, 12, 12, 64, 0), 1),
    ({}, (1, 512, 15, 16, 64, 0), 1),
    ({}, (1, 512, 33, 32, 64, 0), 1),
    ({}, (1, 512, 20, 16, 64, 0), 1),
    ({}, (1, 512, 6, 32, 64, 0), 1),
    ({}, (1, 512, 2, 64, 64, 0), 1),
    ({}, (1, 512, 48, 256, 64, 0), 1),
    # raw widths 16 / 32 / 64 / 128 at one to a few workgroup pairs: split 4 (C = 512), 2 (C = 256), none (C = 64)
    ({}, (1, 512, 16, 16, 64, 0), 4),
    ({}, (1, 256, 16, 16, 64, 0), 2),
    ({}, (1, 64, 16, 16, 64, 0), 1),
    ({}, (1, 512, 32, 16, 64, 0), 4),
    ({}, (1, 512, 8, 32, 64, 0), 4),
    ({}, (1, 512, 32, 32, 64, 0), 4),
    ({}, (1, 256, 32, 32, 64, 0), 2),
    ({}, (1, 512, 4, 64, 64, 0), 4),
    ({}, (1, 512, 64, 64, 64, 0), 4),
    ({}, (1, 512, 2, 128, 64, 0), 4),
    ({}, (1, 512, 6, 128, 64, 0), 4),
    ({}, (1, 512, 128, 128, 64, 0), 4),
    ({}, (1, 64, 128, 128, 64, 0), 1),
    # chunk counts that do not divide: 520 channels = 65 chunks, 528 = 66 (33 per half: odd), 384 = 48 (12 per quarter: < 16)
    ({}, (1, 520, 16, 16, 64, 0), 1),
    ({}, (1, 528, 16, 16, 64, 0), 1),
    ({}, (1, 384, 16, 16, 64, 0), 2),
    ({}, (1, 505, 16, 16, 64, 0), 4),
    # the number of pairs against the 256 compute units
    ({}, (2, 512, 128, 128, 64, 0), 2),
    ({}, (4, 512, 128, 128, 64, 0), 1),
    ({}, (8, 512, 128, 128, 64, 0), 1),
    ({}, (128, 512, 128, 128, 64, 0), 1),
    ({}, (8, 256, 32, 32, 256, 0), 2),
    ({}, (8, 512, 16, 16, 512, 0), 4),
    ({}, (8, 512, 16, 16, 520, 0), 2),
    # output channels: tails 0, 1 .. 4 (thin kernel: the tile is not counted), 5; K <= 4 (no MFMA launch); K = 5 .. 64
    ({}, (1, 512, 128, 128, 128, 0), 2),
    ({}, (1, 512, 128, 128, 65, 0), 4),
    ({}, (1, 512, 128, 128, 67, 0), 4),
    ({}, (1, 512, 128, 128, 68, 0), 4),
    ({}, (1, 512, 128, 128, 69, 0), 2),
    ({}, (1, 512, 128, 128, 131, 0), 2),
    ({}, (1, 512, 128, 128, 259, 0), 1),
    ({}, (1, 512, 128, 128, 1, 0), 1),
    ({}, (1, 512, 128, 128, 3, 0), 1),
    ({}, (1, 512, 128, 128, 4, 0), 1),
    ({}, (1, 512, 128, 128, 5, 0), 4),
    ({}, (1, 512, 128, 128, 63, 0), 4),
    # a fused activation never splits
    ({}, (1, 512, 16, 16, 64, 1), 1),
    ({}, (1, 256, 32, 32, 64, 1), 1),
    # options
    ({"conv_wino_split": 0}, (1, 512, 16, 16, 64, 0), 1),
    ({"conv_wino_split": 2}, (1, 512, 16, 16, 64, 0), 2),
    ({"conv_wino_split": 2}, (1, 256, 16, 16, 64, 0), 2),
    ({"conv_wino_split": 2}, (1, 64, 16, 16, 64, 0), 1),
    ({"conv_wino_split": 1}, (1, 512, 16, 16, 64, 0), 4),
    ({"conv_wino_raw": 0}, (1, 512, 16, 16, 64, 0), 1),
    ({"conv_wino_raw": 0}, (1, 512, 128, 128, 64, 0), 1),
    ({"conv_thin_tail": 0}, (1, 512, 128, 128, 67, 0), 2),
    ({"conv_thin_tail": 0}, (1, 512, 128, 128, 3, 0), 4),
    ({"conv_thin_tail": 0}, (1, 512, 128, 128, 64, 0), 4),
    ({"conv_wino_ws": 1}, (1, 512, 16, 16, 64, 0), 4),
    # invalid sizes: "no split"
    ({}, (0, 512, 16, 16, 64, 0), 1),
    ({}, (1, 512, 16, 16, 0, 0), 1),
    ({}, (1, -1, 16, 16, 64, 0), 1),
]

# ((K, C), bytes)
WINO_WORKSPACE = [
    ((64, 64), 262144), ((64, 8), 32768), ((1, 1), 32768), ((3, 195), 819200), ((67, 70), 589824), ((65, 9), 131072),
    ((195, 195), 3276800), ((512, 512), 16777216), ((520, 505), 18874368), ((0, 5), 0), ((5, 0), 0), ((-1, 8), 0),
]

# ({option: value}, (B, C, H, W, K, kernel, stride, pad, mode), bytes; -1 = invalid arguments)
CONV_FWD_WORKSPACE = [
    # mode 0 (convolution), 3 x 3 and 4 x 4, stride 1 and 2: few tiles split, >= 256 tiles do not
    ({}, (6, 256, 8, 8, 512, 3, 1, 1, 0), 12582912),
    ({}, (6, 256, 8, 8, 512, 3, 2, 1, 0), 3145728),
    ({}, (6, 512, 4, 4, 1024, 3, 1, 1, 0), 3145728),
    ({}, (6, 128, 32, 32, 256, 3, 2, 1, 0), 12582912),
    ({}, (2, 64, 8, 8, 64, 4, 2, 1, 0), 262144),
    ({}, (2, 64, 8, 8, 64, 4, 1, 1, 0), 802816),
    ({}, (8, 64, 64, 64, 256, 3, 1, 1, 0), 0),
    ({}, (32, 64, 64, 64, 128, 3, 1, 1, 0), 0),
    ({}, (1, 3, 16, 16, 8, 3, 1, 1, 0), 0),
    ({}, (1, 4, 8, 8, 64, 3, 1, 1, 0), 0),
    # mode 1: ConvTranspose2d(4, 2, 1)
    ({}, (6, 512, 4, 4, 256, 4, 2, 1, 1), 3145728),
    ({}, (6, 1024, 2, 2, 512, 4, 2, 1, 1), 1572864),
    ({}, (6, 64, 64, 64, 32, 4, 2, 1, 1), 0),
    ({}, (32, 128, 64, 64, 256, 4, 2, 1, 1), 0),
    # mode 2: d(input) of Conv2d(3, 2, 1); mode 3: of Conv2d(3, 1, 1)
    ({}, (6, 512, 4, 4, 256, 3, 2, 1, 2), 3145728),
    ({}, (2, 64, 8, 8, 32, 3, 2, 1, 2), 524288),
    ({}, (32, 256, 64, 64, 256, 3, 2, 1, 2), 0),
    ({}, (6, 512, 8, 8, 256, 3, 1, 1, 3), 12582912),
    ({}, (2, 32, 8, 8, 64, 3, 1, 1, 3), 262144),
    ({}, (32, 128, 64, 64, 256, 3, 1, 1, 3), 0),
    # <= 96 output pixels per class: the target of 256 workgroups
    ({}, (1, 512, 8, 8, 512, 3, 1, 1, 0), 4194304),
    ({}, (6, 512, 4, 4, 512, 3, 1, 1, 0), 3145728),
    ({}, (6, 1024, 2, 2, 1024, 3, 1, 1, 0), 1572864),
    # options: the split target, the tile shape
    ({"conv_fwd_split_target": 128}, (6, 256, 8, 8, 512, 3, 1, 1, 0), 2359296),
    ({"conv_fwd_split_target": 2048}, (6, 256, 8, 8, 512, 3, 1, 1, 0), 25165824),
    ({"conv_fwd_split_target": 100000}, (6, 256, 8, 8, 512, 3, 1, 1, 0), 50331648),
    ({"conv_fwd_split_target": 512}, (6, 512, 4, 4, 256, 4, 2, 1, 1), 6291456),
    ({"conv_tile_variant": 1}, (6, 256, 8, 8, 512, 3, 1, 1, 0), 12582912),
    ({"conv_tile_variant": 2}, (6, 256, 8, 8, 512, 3, 1, 1, 0), 25165824),
    ({"conv_tile_variant": 3}, (6, 256, 8, 8, 512, 3, 1, 1, 0), 25165824),
    ({"conv_tile_variant": 4}, (6, 256, 8, 8, 512, 3, 1, 1, 0), 50331648),
    ({"conv_tile_variant": 1}, (8, 64, 64, 64, 256, 3, 1, 1, 0), 0),
    # invalid arguments
    ({}, (0, 64, 8, 8, 64, 3, 1, 1, 0), -1),
    ({}, (1, 64, 8, 8, 64, 3, 1, 1, 4), -1),
    ({}, (1, 64, 8, 8, 64, 3, 1, 1, -1), -1),
    ({}, (1, 64, 8, 8, 64, 5, 1, 1, 0), -1),
    ({}, (1, 64, 8, 8, 64, 3, 3, 1, 0), -1),
    ({}, (1, 64, 8, 8, 64, 3, 1, 3, 0), -1),
    ({}, (1, 64, 8, 8, 64, 3, 2, 1, 1), -1),
    ({}, (1, 64, 8, 8, 64, 4, 2, 1, 2), -1),
    ({}, (1, 64, 8, 8, 64, 4, 1, 1, 3), -1),
    ({}, (1, 64, 8, 8, 64, 3, 2, 1, 3), -1),
    ({}, (1, 64, 1, 1, 64, 4, 1, 0, 0), -1),
    ({}, (1048576, 64, 64, 64, 64, 3, 1, 1, 0), -1),
]


def _ids(rows):
    return ["%s%s" % ("x".join(str(v) for v in r[1]), "".join(" %s=%d" % kv for kv in sorted(r[0].items())) if len(r) == 3 else "")
            for r in rows]


@pytest.mark.parametrize("opts,args,expected", WINO_SPLITS, ids=_ids(WINO_SPLITS))
def test_winograd_splits(hiplib, options, opts, args, expected):
    for k, v in opts.items():
        options(k, v)
    assert hiplib.ffwm_conv3x3_winograd_splits(*args) == expected


def test_winograd_workspace_bytes(hiplib):
    got = [(a, hiplib.ffwm_conv3x3_winograd_workspace_bytes(*a)) for a, _ in WINO_WORKSPACE]
    assert got == WINO_WORKSPACE


@pytest.mark.parametrize("opts,args,expected", CONV_FWD_WORKSPACE, ids=_ids(CONV_FWD_WORKSPACE))
def test_conv2d_forward_workspace(hiplib, options, opts, args, expected):
    for k, v in opts.items():
        options(k, v)
    assert hiplib.ffwm_conv2d_forward_workspace(*args) == expected


def test_options_are_restored(hiplib):
    """The rows above leave every option they set at its default."""
    for name, default in (("conv_wino_split", 1), ("conv_wino_raw", 1), ("conv_thin_tail", 1), ("conv_wino_ws", 0),
                          ("conv_fwd_split_target", 0), ("conv_tile_variant", 0)):
        assert hiplib.ffwm_set_option(name.encode(), default) == default
