"""Sequential long-form in Python: the seek rule and the loop of host/wh_host.h (seek_advance, run_sequential), restated from
openai-whisper's transcribe() without word_timestamps.  The tests compare the C++ against this; nothing here calls the code under test."""
import math

WINDOW_FRAMES = 3000
RESET_TEMPERATURE = 0.5     # openai-whisper: a window decoded above this does not condition the next one


def seek_advance(generated, tb, eot, seg_frames):
    """-> (segments [{"start", "end", "ids"}], advance in frames) of one window's generated ids."""
    g = []
    for x in generated:
        if x == eot:
            break
        g.append(int(x))
    n = len(g)
    ts = [x >= tb for x in g]
    cuts = [i for i in range(1, n) if ts[i - 1] and ts[i]]
    segs = []
    if cuts:
        single_end = n >= 2 and not ts[n - 2] and ts[n - 1]
        advance = seg_frames if single_end else (g[cuts[-1] - 1] - tb) * 2
        if single_end:
            cuts = cuts + [n]
        last = 0
        for c in cuts:
            start = (g[last] - tb) * 0.02 if ts[last] else 0.0      # (a slice that opens with text: from 0; the timestamp rules never produce one)
            segs.append({"start": start, "end": (g[c - 1] - tb) * 0.02, "ids": g[last:c]})
            last = c                                                  # text after the last cut is no segment: the next window decodes it again
    else:
        end = seg_frames * 0.01
        stamps = [x for x in g if x >= tb]
        if stamps and stamps[-1] != tb:
            end = (stamps[-1] - tb) * 0.02
        segs.append({"start": 0.0, "end": end, "ids": list(g)})
        advance = seg_frames
    segs = [s for s in segs if s["start"] != s["end"] and any(x < tb for x in s["ids"])]
    if advance == 0:            # the deviation: a closing pair at <|0.00|> would never terminate
        advance = seg_frames
    return segs, advance


def skip_window(no_speech_prob, avg_lp, no_speech_threshold, logprob_threshold):
    if no_speech_threshold is None or not (no_speech_prob > no_speech_threshold):
        return False
    return logprob_threshold is None or avg_lp < logprob_threshold


def prefix_of(history, reset_since, sot_prev, n_text_ctx, n_prompt, max_new_tokens):
    """[sot_prev] ++ the last n_text_ctx / 2 - 1 ids of the live history, the oldest dropped until prefix + prompt + generated fit the text context."""
    live = history[reset_since:]
    if not live:
        return []
    keep = min(len(live), max(n_text_ctx // 2 - 1, 0))
    room = n_text_ctx - n_prompt - max_new_tokens
    if 1 + keep > room:
        if room < 2:
            return []
        keep = room - 1
    return [sot_prev] + live[len(live) - keep:] if keep else [sot_prev]


def run_sequential(frames, step, tb, eot, sot_prev, n_text_ctx, n_prompt, max_new_tokens, condition_on_previous_text=True,
                   no_speech_threshold=None, logprob_threshold=None, initial_prompt=()):
    """step(rows) with rows = [{"file", "window", "seek", "seg_frames", "prefix"}] in file order returns one {"tokens", "avg_logprob",
    "no_speech_prob", "temperature"} per row.  -> {"steps": [[files]], "files": [{"windows": [...], "segments": [...]}]}."""
    n = len(frames)
    seek = [0] * n
    history = [list(initial_prompt) for _ in range(n)]
    reset_since = [0] * n
    files = [{"windows": [], "segments": []} for _ in range(n)]
    steps = []
    while True:
        rows = []
        for f in range(n):
            if seek[f] >= frames[f]:
                continue
            rows.append({"file": f, "window": len(files[f]["windows"]), "seek": seek[f], "seg_frames": min(WINDOW_FRAMES, frames[f] - seek[f]),
                         "prefix": prefix_of(history[f], reset_since[f], sot_prev, n_text_ctx, n_prompt, max_new_tokens)})
        if not rows:
            break
        steps.append([r["file"] for r in rows])
        res = step(rows)
        assert len(res) == len(rows)
        for r, x in zip(rows, res):
            f = r["file"]
            temp = float(x.get("temperature", 0.0))
            w = {"seek": r["seek"], "seg_frames": r["seg_frames"], "tokens": [int(t) for t in x["tokens"]], "prefix": r["prefix"], "temperature": temp}
            if skip_window(x.get("no_speech_prob", 0.0), x.get("avg_logprob", 0.0), no_speech_threshold, logprob_threshold):
                w["skipped"], w["advance"] = True, r["seg_frames"]          # (openai-whisper `continue`s: history and reset_since stay)
            else:
                segs, adv = seek_advance(x["tokens"], tb, eot, r["seg_frames"])
                w["skipped"], w["advance"] = False, adv
                for s in segs:
                    files[f]["segments"].append({"start": s["start"] + r["seek"] * 0.01, "end": s["end"] + r["seek"] * 0.01, "ids": s["ids"]})
                    history[f] += s["ids"]
                if not condition_on_previous_text or temp > RESET_TEMPERATURE:
                    reset_since[f] = len(history[f])
            seek[f] += w["advance"]
            files[f]["windows"].append(w)
    return {"steps": steps, "files": files}


def scripted_step(script):
    """The step of a scripted run: file f's window k decodes to script[f][min(k, len - 1)]."""
    def step(rows):
        return [script[r["file"]][min(r["window"], len(script[r["file"]]) - 1)] for r in rows]
    return step
