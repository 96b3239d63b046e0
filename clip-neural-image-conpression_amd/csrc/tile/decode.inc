// Workgroup decode.  blockIdx.x = (((b * n_ty + ty) * n_tx + tx) * npar + par) * n_nt + nt: the channel tiles of one pixel tile
// are neighbours.  Expects: a, TH, BN.  Defines: nt, par, tx, ty, b; my0, mx0 (first M-space row / column), n0 (first output
// channel); py, px_ (ConvTranspose output parity), par_off (its first entry of ConvArgs::tapinfo).
    int bid = blockIdx.x;
    const int nt = bid % a.n_nt; bid /= a.n_nt;
    const int par = bid % a.npar; bid /= a.npar;
    const int tx = bid % a.n_tx; bid /= a.n_tx;
    const int ty = bid % a.n_ty;
    const int b = bid / a.n_ty;
    const int my0 = ty * TH, mx0 = tx * 32, n0 = nt * BN;
    const int py = par >> 1, px_ = par & 1;
    const int par_off = par * 4;
