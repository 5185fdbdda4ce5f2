function y = emaglsResample(x, p, q)
% MATLAB's resample(x, p, q) with its defaults (N = 10, bta = 5) on the GPU, for users without the Signal Processing Toolbox:
% own restatement of resample.m (DESIGN.md section 7), so MATLAB's exact tap values are not guaranteed.  p and q are positive
% integers; a row vector is resampled along its length, a matrix per column; real or complex.  The result has
% ceil(size(x, 1) * p / q) rows (columns for a row vector).  Named so as not to shadow the toolbox's resample.
y = emagls_mex('resample', double(x), double(p), double(q));
end
