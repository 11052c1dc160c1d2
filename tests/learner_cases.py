"""TEST INFRASTRUCTURE — the case sets of the fused learner's exact tests (tests/test_gpu_loss_exact.py and the distill
tests built on it): sizes, weight-set names, sentinels, the exact forward of a case, the Learner that drives
tarok_learn_chain over guarded buffers, and the rollout words of tests/test_gpu_learner.py."""
import numpy as np

import loss_model as L
from policy_exact_ref import P_PARAMS, check_conditions_p, check_conditions_r, reference, synthetic_features, weights_p, weights_r


M, SEED = 333, 17                          # the case set of the chain (and of tarok_ppo_loss at n = 333)
N2, SEED2 = 257, 18                        # tarok_ppo_loss: one full block of 256 and one sample
# one tile of k_learn_chain is 96 samples: a ragged tile, one full tile, a full tile plus one sample, three tiles plus 45
CONFIGS = ((33, True), (33, False), (96, True), (96, False), (97, True), (97, False), (333, True), (333, False))   # (B, through an index)
P_A, P_B = 2, 8                            # the two sets P (indices into P_PARAMS)
SETS = ("R", "P%d" % P_A, "P%d" % P_B)
SENTINEL_BF16 = 0x7FC1                     # (as in test_gpu_learner.py: a NaN payload no kernel writes)
SENTINEL_WORD = 0x5A5A5A5A5A5A5A5A


def weight_set(name):
    return weights_r() if name == "R" else weights_p(*P_PARAMS[int(name[1:])])


def forward_of(name, x):
    """The exact forward of feature rows x (numpy [n,256]) under a weight set, its conditions re-checked on these rows."""
    import torch
    W = weight_set(name)
    r = reference(torch.from_numpy(x), W)
    if name == "R":
        check_conditions_r(r, W)
    else:
        check_conditions_p(r, W)
    return W, r


def features(n, seed):
    cases = L.build_cases(n, seed, "mixed")
    return L.features_with_masks(synthetic_features(n, seed).numpy(), cases["legal"]), cases["masks"]


def subset_reference(cases, logits, logp_old, rows):
    clip, vf, ent = L.MODES[cases["mode"]]
    return L.loss_reference(logits[rows], cases["legal"][rows], cases["card"][rows], logp_old[rows].astype(np.float64),
                            cases["A"][rows], cases["ret"][rows], cases["known"][rows].astype(np.float64), clip, vf, ent)


class Learner:
    """The fused learner's buffers for one weight set: the weights go in through learn_adam(..., apply=False)."""

    def __init__(self, T, W):
        import torch
        K = T.karte
        self.T, self.K = T, K
        self.env = T.TarokVecEnv(256, seed=1)
        flat = torch.cat([t.reshape(-1) for t in W]).float().cuda().contiguous()
        assert flat.numel() == K.MLP_PARAMS, "not true: flat.numel() == K.MLP_PARAMS"
        bf = lambda k: torch.empty(k, dtype=torch.bfloat16, device="cuda")
        self.wf = dict(w1=bf(65536), w2=bf(65536), w3=bf(16384), w3t=bf(16384), w2t=bf(65536))
        self.env.learn_adam(flat, None, None, None, None, self.wf, apply=False)
        self.bias = (flat[K.MLP_B1:K.MLP_B1 + 256], flat[K.MLP_B2:K.MLP_B2 + 256], flat[K.MLP_B3:K.MLP_B3 + 64])
        self.flat = flat

    def chain(self, B, words, idx, rec, stats, mode):
        """One tarok_learn_chain launch; returns the arrays' first B rows as float64 numpy, whether every padding row kept
        its sentinel, the gathered feature words and the four terms (float32)."""
        import torch
        K = self.K
        clip, vf, ent = L.MODES[mode]
        act_t = lambda k: torch.zeros((B + K.LEARN_PAD, k), dtype=torch.bfloat16, device="cuda")
        arr = dict(H1=act_t(256), H2=act_t(256), dH2=act_t(256), dH1=act_t(256), dOut=act_t(64))
        for t_ in arr.values():
            t_[B:].view(torch.int16).fill_(SENTINEL_BF16)
        Xw = torch.zeros((B + K.LEARN_PAD, 4), dtype=torch.int64, device="cuda")
        Xw[B:] = SENTINEL_WORD
        scratch = torch.empty(((B + 95) // 96, 4), device="cuda")
        terms = torch.empty(4, device="cuda")
        self.env.learn_chain(B, words, idx, rec, stats, clip, vf, ent, self.wf, self.bias, Xw, arr["H1"], arr["H2"], arr["dOut"],
                             arr["dH2"], arr["dH1"], scratch, terms)
        torch.cuda.synchronize()
        out = {k: v[:B].double().cpu().numpy() for k, v in arr.items()}
        out["pads"] = {k: bool((v[B:].view(torch.int16) == SENTINEL_BF16).all().item()) for k, v in arr.items()}
        out["pads"]["Xw"] = bool((Xw[B:] == SENTINEL_WORD).all().item())
        out["Xw"] = Xw[:B].cpu().numpy()
        out["terms"] = terms.cpu().numpy()
        return out

    def close(self):
        self.env.close()


def _rollout_words(T, env, net_w, steps):
    """feature words [steps * n, 4] and observation words of real positions (policy_mlp on a stepped env)"""
    import torch
    obs = env.reset()
    fws, ows = [], []
    for t in range(steps):
        for _ in range(3):
            obs, _, _ = env.step(env.policy_random(obs), auto_reset=True)
        fw = torch.zeros((env.n, 4), dtype=torch.int64, device="cuda")
        env.policy_mlp(net_w, obs.words, feature_words_out=fw)
        fws.append(fw); ows.append(obs.words.clone())
    return torch.cat(fws), torch.cat(ows)
