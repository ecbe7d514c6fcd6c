"""The long-context inputs that tests/test_semantic_decoder_edges_gpu.py runs and tests/test_oracle_gpt_cpu.py qualifies, in one place so that both use the
very same ids. A case is a seeded prompt plus ``max_new`` generated ids that the allow ranges force (even steps may produce FORCED[0] only, odd steps
FORCED[1]), so the whole sequence is known without a device and the CPU test can show, at exactly the positions the GPU test compares, that a
kernel which lost one key, shifted the positions or lost a token's K/V would move the logits by many times the float bar."""
import numpy as np

V = 2048
FORCED = (701, 1402)
FORCED_ALLOW = [[FORCED[0], FORCED[0] + 1, 0, 0], [FORCED[1], FORCED[1] + 1, 0, 0]]
BLOCK = 1024

# name: prompt length, max_new, the ids the call can produce (the block ends the longest case after 24), and the mutants the CPU test qualifies:
#   ("mask", query, key)   that query does not see that key (one per 256-key slot of gpt_attn_kernel's s[0..3], and both sides of 512 and 768)
#   ("wpe", p)             every position from p on takes the next position's embedding
#   ("kv", j)              prompt token j's K and V are zero in every layer and head
LONG_CASES = {
    "cross_512": dict(plen=505, max_new=16, produced=16,
                      mutants=[("mask", 512, 512), ("mask", 512, 511), ("mask", 519, 256), ("mask", 504, 3), ("wpe", 300), ("kv", 100)]),
    "cross_768": dict(plen=761, max_new=16, produced=16,
                      mutants=[("mask", 768, 768), ("mask", 768, 767), ("mask", 768, 511), ("mask", 775, 0), ("wpe", 770), ("kv", 600)]),
    "longest": dict(plen=1000, max_new=64, produced=24,
                    mutants=[("mask", 1022, 1022), ("mask", 1022, 768), ("mask", 1022, 1000), ("wpe", 1010), ("kv", 999)]),
}


def long_prompt(plen):
    return np.random.default_rng(plen).integers(0, V, size=plen).astype(np.int32)


def long_sequence(name):
    """(prompt + the forced ids, the positions whose logits the GPU test compares: one per produced id)."""
    c = LONG_CASES[name]
    forced = np.array([FORCED[s % 2] for s in range(c["produced"])], dtype=np.int32)
    P = c["plen"]
    return np.concatenate([long_prompt(P), forced]), list(range(P - 1, P - 1 + c["produced"]))
