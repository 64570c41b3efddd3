"""The kmeans score on the host: the method / config surface and the entry points' checks."""
import ctypes

import pytest

from data_diet_distributed_amd import _capi, config, methods
from data_diet_distributed_amd.forward_scores import kmeans_seed_rows
from data_diet_distributed_amd.scoring import ScoreConfig


def test_method_and_config_surface():
    assert methods.CLUSTER_METHODS == ("kmeans",)
    assert methods.known("kmeans") and methods.pass_of("kmeans") == "el2n"
    assert not methods.refinable("kmeans")
    assert config.DEFAULTS["kmeans_k"] == 0 and config.DEFAULTS["kmeans_iters"] == 20
    cfg = ScoreConfig(methods=("el2n", "kmeans"), select_by="kmeans", kmeans_k=4096)
    assert (cfg.kmeans_k, cfg.kmeans_iters) == (4096, 20)
    for kw in ({"kmeans_k": -1}, {"kmeans_k": 4097}, {"kmeans_iters": 0}, {"kmeans_iters": 1001},
               {"kmeans_k": True}):
        with pytest.raises(ValueError, match="kmeans_"):
            ScoreConfig(methods=("kmeans",), select_by="kmeans", **kw)
        ScoreConfig(**kw)  # validated only when kmeans is requested
    assert _capi.KMEANS_MAX_K == 4096 and _capi.lib().dd_abi_version() == 10
    assert kmeans_seed_rows(301, 4) == [37, 112, 188, 263] and kmeans_seed_rows(7, 1) == [3]


def test_workspace_bytes():
    wb = _capi.kmeans_workspace_bytes
    # the halves of every row and centroid, a norm and an int64 id per centroid, in 256-byte units
    assert wb(256, 64, 64) == 4 * (256 + 64) * 64 + 4 * 64 + 8 * 64
    assert wb(256, 64, 49) == wb(256, 64, 64) and wb(0, 1, 1, "bf16x3") == 4 * 256
    L = _capi.lib()
    for bad in ((4, 2, 0, 1), (4, 2, 4097, 1), (4, 0, 8, 1), (4, 4097, 8, 1), (4, 2, 8, 2),
                (4, 2, 8, -1), (-1, 2, 8, 1), (1 << 31, 2, 8, 1)):
        assert L.dd_kmeans_workspace_bytes(*bad) == 0, bad


def test_entry_points_validate_before_launching():
    """DD_EINVAL and a message before any device work (so this runs without a GPU)."""
    L = _capi.lib()
    P16 = ctypes.c_void_p(16)

    def call(n=4, Kc=2, D=8, operands=1, rows=P16, cent=P16, sums=P16, counts=P16, bad=P16,
             assign=P16, dist=P16, accum=P16, ws=P16, ws_bytes=1 << 30):
        return L.dd_kmeans_assign(rows, n, cent, Kc, D, operands, 1, sums, counts, bad, assign,
                                  dist, accum, ws, ws_bytes, None)

    nothing = {"sums": None, "counts": None, "assign": None, "dist": None, "accum": None}
    for kw, word in (({"Kc": 0}, b"<= Kc"), ({"Kc": 4097}, b"<= Kc"), ({"D": 0}, b"<= D"),
                     ({"n": 1 << 31}, b"<= n"), ({"operands": 2}, b"operands"),
                     (nothing, b"no output"), ({"counts": None}, b"go together"),
                     ({"rows": None}, b"null"), ({"cent": None}, b"null"), ({"bad": None}, b"null"),
                     ({"ws": None}, b"workspace"), ({"ws_bytes": 64}, b"workspace"),
                     ({"ws": ctypes.c_void_p(24)}, b"aligned")):
        assert call(**kw) == -1, kw
        err = L.dd_last_error()
        assert err.startswith(b"dd_kmeans_assign") and word in err, (kw, err)
    assert call(n=0, rows=None, ws=None, ws_bytes=0) == 0 and L.dd_last_error() == b""
    assert L.dd_kmeans_centroids(P16, P16, 0, 8, P16, None) == -1
    assert L.dd_kmeans_centroids(None, P16, 2, 8, P16, None) == -1
    assert L.dd_last_error().startswith(b"dd_kmeans_centroids")
