"""surrogate="gbt" through the driver on a small mixed space: the boosted
ensemble is refitted as results arrive, only unseen configurations are
proposed, and a round's selections are the top-k of -pred recomputed on the
host from the records ut_forest_get returns.  Needs a GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

import _rf_fit_oracle as RF  # noqa: E402
from test_gpu_tpe_technique import _cost, _space  # noqa: E402  (the small mixed space)


def test_technique_refits_proposes_unseen_and_selects_the_top_k_of_its_prediction():
    from uptune_amd import technique as T
    from uptune_amd.driver import SearchDriver
    de = T.GpuDifferentialEvolution(surrogate="gbt", gbt_kw={"n_rounds": 20, "max_depth": 4}, pool=2048, batch=4,
                                    seed=5)
    d = SearchDriver(_space(), de, parallelism=4)
    d.main(_cost, test_limit=16)   # four rounds of four
    de = d.root_technique   # the driver's own copy
    model, eng = de.model, de.model.engine
    hist = [r.configuration.hash for r in d.results.values()]
    assert len(hist) >= 16 and len(set(hist)) == len(hist)
    assert model.fits > 1 and model.fit_seconds > 0
    roots, nodes = eng.forest_get()
    assert roots.size == 20

    # one more round by hand: the same steps as GpuBatchTechnique._local_round
    assert model.fit(d)
    roots, nodes = eng.forest_get()
    vals, invalid = de.propose(de.pool)
    dup = eng.dedup(de.hash_proposals(vals, de.round_base()))
    if invalid is not None:
        dup = torch.maximum(dup, invalid)
    feat = eng.encode(vals)
    pred, score = eng.forest_predict(feat, dup=dup)
    fh = feat.cpu().numpy()[:, :vals.shape[1]].T
    leaf = RF.route(nodes, roots, RF.codes_of(fh))
    want = np.full(fh.shape[0], float(np.mean(model._transform(model._ya[:model._n]))))
    for t in range(len(roots)):
        want = want + nodes["value"][leaf[:, t]]
    np.testing.assert_array_equal(pred.cpu().numpy().view(np.int64), want.view(np.int64))
    host_score = np.where(dup.cpu().numpy() != 0, -np.inf, -want)
    idx, top = eng.topk(score, de.batch)
    order = np.lexsort((np.arange(host_score.size), -host_score))[:de.batch]   # ties to the lower index
    np.testing.assert_array_equal(np.sort(idx.cpu().numpy()), np.sort(order))
    np.testing.assert_array_equal(top.cpu().numpy(), host_score[idx.cpu().numpy()])
