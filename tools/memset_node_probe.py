"""Does a hipMemsetAsync node of a captured graph clear its buffer on EVERY replay?  (why finrom_romml_grad clears info
with a kernel.)  No library code: a graph of three [kernel, memset of `count` int32, kernel, copy of the buffer aside] groups on
one buffer, refilled with 5 before each of three replays; prints, per replay, which of the three copies saw zeros.  Sizes are the
info buffers of 4, 64, 65 and 70 chains, in torch memory and in hipMalloc memory.

    python tools/memset_node_probe.py"""
import ctypes as C

import torch

hip = C.CDLL("libamdhip64.so.7", mode=4)                 # the runtime torch has loaded (RTLD_NOLOAD)
hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipFree.argtypes = [C.c_void_p]
PAD, NODES, D2D = 8, 3, 3


def trial(count, own_malloc):
    n = count + PAD
    own, info = C.c_void_p(), None
    if own_malloc:
        assert hip.hipMalloc(C.byref(own), 4 * n) == 0
        ptr = own.value
    else:
        info = torch.full((n,), 5, dtype=torch.int32, device="cuda")
        ptr = info.data_ptr()
    fives = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    seen = torch.zeros((NODES, n), dtype=torch.int32, device="cuda")
    work = torch.zeros(4096, device="cuda")

    def copy(dst, src):
        assert hip.hipMemcpyAsync(dst, src, 4 * n, D2D, torch.cuda.current_stream().cuda_stream) == 0

    def body():
        for i in range(NODES):
            work.add_(1.0)
            assert hip.hipMemsetAsync(ptr, 0, 4 * count, torch.cuda.current_stream().cuda_stream) == 0
            work.mul_(1.0)
            copy(seen[i].data_ptr(), ptr)                    # what a kernel behind the memset would read
            if info is not None:
                info[:count].add_(7)                         # a later kernel flags every entry again

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    for replay in range(3):
        copy(ptr, fives.data_ptr())
        seen.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        s = seen.cpu().numpy()
        print("hipMalloc" if own_malloc else "torch", "memory,", 4 * count, "bytes, replay", replay, ": cleared behind node 0 / 1 / 2:",
              [bool((s[i, :count] == 0).all()) for i in range(NODES)], "padding kept:", bool((s[:, count:] == 5).all()), flush=True)
    del g
    torch.cuda.synchronize()
    if own_malloc:
        hip.hipFree(own)


if __name__ == "__main__":
    for count in (4, 64, 65, 70):
        trial(count, False)
    for count in (4, 65):
        trial(count, True)
