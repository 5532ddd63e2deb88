"""numpy restatement of rsr_sequence_sources (include/realsr_hip.h "frame sequences"): for every output tile of every frame of a window,
the frame whose computed rectangle it shows.  Plain loops; nothing here shares code with the library."""
import numpy as np


def sources(masks, has_prev):
    """masks: (n, ntiles), any non-zero byte is set.  Returns the int (n, ntiles) array src: src[k, t] = k where masks[k, t] is set, else
    the largest j < k with masks[j, t] set, else -1 (the previous output).  ValueError where a -1 is needed and has_prev is false."""
    masks = np.asarray(masks)
    n, ntiles = masks.shape
    src = np.zeros((n, ntiles), dtype=np.int64)
    for k in range(n):
        for t in range(ntiles):
            s = -1
            for j in range(k + 1):
                if masks[j, t] != 0:
                    s = j
            if s < 0 and not has_prev:
                raise ValueError("tile %d of frame %d has no source" % (t, k))
            src[k, t] = s
    return src
