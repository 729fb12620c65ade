"""In-process A/B of BASELINE config 3's decode (device-resident, (10,5,2), 360 000 packets of
bin/erasure.bin) over environment switches the library reads per launch (one under trial in a
working tree), alternating variants:
    python tools/config3_ab.py FEC_X=1024 FEC_X=4096,FEC_Y=1 [rounds]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from fec_erasure_code_unit_test_relay_amd import Codec, fill_payload  # noqa: E402
from fec_erasure_code_unit_test_relay_amd.streams import load_pattern  # noqa: E402

args = [a for a in sys.argv[1:] if "=" in a]
rounds = int(next((a for a in sys.argv[1:] if "=" not in a), "6"))
L, P = 300, 360000
torch.cuda.set_device(0)
pat = load_pattern("bin_erasure")
c = Codec(L, 10, 5, 2)
payload = fill_payload(0, P + 10, L, 0x5EED)
cw, _ = c.encode(payload)
er = torch.from_numpy(pat[:P + 10].copy()).cuda()
out = torch.empty((P, L), dtype=torch.uint8, device="cuda")
ol = torch.empty(P, dtype=torch.int32, device="cuda")
c.workspace(P + 10)
res = {a: [] for a in args}
for _ in range(rounds):
    for a in args:
        for kv in a.split(","):  # K=V[,K2=V2]: every variant names all its switches
            k, v = kv.split("=", 1)
            os.environ[k] = v
        for _ in range(3):
            c.decode(cw, er, out=out, out_len=ol)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            c.decode(cw, er, out=out, out_len=ol)
        torch.cuda.synchronize()
        res[a].append((time.perf_counter() - t0) / 20 * 1e3)
        lost = int((ol == 0).sum())
        assert lost == 565, (a, lost)
for a in args:
    print(f"{a:28s} median {statistics.median(res[a]):.4f} ms  all {' '.join(f'{x:.4f}' for x in res[a])}")
