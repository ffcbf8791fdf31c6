"""Pure-Python statement of the test-time-augmentation pick rule (avec_ctc_tta_pick, include/avec_hip.h), on nested lists.

tokens [S][W][T], out_len [S][W], score [S][W] are the outputs of the beam search on S = B * n rows, row b * n + k = augmentation k of utterance b.
Without best_slot the winner of utterance b is the augmentation whose slot-0 score is highest, scanned from augmentation 0 with a strict > (ties, and an utterance
whose slots are all -inf, go to the lower index), and beam 0.  With best_slot it is slot clamp(best_slot[b], 0, n * W - 1) = augmentation * W + beam.
ids = the winner's tokens, zero at and past ids_len = its out_len clamped to [0, T], and 0 when its score is -inf."""

NEG_INF = float("-inf")


def pick(tokens, out_len, score, n, best_slot=None):
    S, W, T = len(tokens), len(tokens[0]), len(tokens[0][0])
    assert S % n == 0
    B = S // n
    best_aug, best_beam, ids, ids_len, best_score = [], [], [], [], []
    for b in range(B):
        if best_slot is None:
            aug, beam, top = 0, 0, score[b * n][0]
            for k in range(1, n):
                if score[b * n + k][0] > top:
                    aug, top = k, score[b * n + k][0]
        else:
            aug, beam = divmod(min(max(int(best_slot[b]), 0), n * W - 1), W)
        s = b * n + aug
        sc = score[s][beam]
        length = min(max(int(out_len[s][beam]), 0), T) if sc > NEG_INF else 0
        best_aug.append(aug)
        best_beam.append(beam)
        ids.append([int(tokens[s][beam][t]) if t < length else 0 for t in range(T)])
        ids_len.append(length)
        best_score.append(sc)
    return best_aug, best_beam, ids, ids_len, best_score
