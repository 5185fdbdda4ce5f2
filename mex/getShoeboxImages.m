function [sources, exponents, paths, emission] = getShoeboxImages(roomDim, sourcePos, arrayPos, fs, maxDelay, varargin)
% The image sources of a shoebox room without its walls, enumerated on the MI355X library (DESIGN.md section 13; include/emagls.h,
% emagls_shoebox_images): every image within maxOrder and maxDelay, for walls that are reflection spectra.
%   [sources, exponents, paths] = getShoeboxImages(roomDim, sourcePos, arrayPos, fs, maxDelay, 'maxOrder', n)
%   roomDim, sourcePos, arrayPos, maxDelay, maxOrder as in getShoeboxComponents
%   sources         cell of Q arrays [J_q x 4] with the columns azimuth, zenith, delay in samples and gain = 1/distance: the lists of
%                   getShoeboxComponents with all six coefficients 1
%   exponents       cell of Q arrays [J_q x 6]: how often each image met the walls x=0, x=Lx, y=0, y=Ly, z=0, z=Lz
%   paths           cell of Q arrays [J_q x 1]: the distances in metres
%   emission        (fourth output, on request) cell of Q arrays [J_q x 3]: the emission vectors, as getShoeboxComponents returns them
%   -- the sources, exponents and pathLength of getArrayIrs with a surfaceReflection of six rows
p = struct('maxOrder', []);
for i = 1:2:numel(varargin)
    if ~isfield(p, varargin{i}); error('eMagLS:arg', 'unknown option "%s"', varargin{i}); end
    p.(varargin{i}) = varargin{i + 1};
end
if size(sourcePos, 2) ~= 3; error('eMagLS:arg', 'sourcePos must be [Q x 3]'); end
args = {'shoebox_images', double(roomDim(:)), double(sourcePos), double(arrayPos(:)), double(fs), double(maxDelay), double(p.maxOrder)};
if nargout > 3
    [compPtr, comps, exps, len, emit] = emagls_mex(args{:});
else
    [compPtr, comps, exps, len] = emagls_mex(args{:});
end
Q = size(sourcePos, 1);
sources = cell(Q, 1);
exponents = cell(Q, 1);
paths = cell(Q, 1);
emission = cell(Q, 1);
for q = 1:Q
    rows = compPtr(q) + 1:compPtr(q + 1);
    sources{q} = comps(rows, :);
    exponents{q} = exps(rows, :);
    paths{q} = len(rows);
    if nargout > 3; emission{q} = emit(rows, :); end
end
end
