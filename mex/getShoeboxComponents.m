function [sources, distances, emission] = getShoeboxComponents(roomDim, wallReflection, sourcePos, arrayPos, fs, maxDelay, varargin)
% The image sources of a shoebox room as plane-wave components at the array's centre, enumerated on the MI355X library (DESIGN.md
% section 12; include/emagls.h, emagls_shoebox_components): Allen & Berkley's image model with frequency-independent walls.
%   sources = getShoeboxComponents(roomDim, wallReflection, sourcePos, arrayPos, fs, maxDelay, 'maxOrder', n)
%   roomDim         [Lx Ly Lz] in metres; one corner at the origin, the axes of getSH (x front, y left, z up)
%   wallReflection  six real amplitude reflection coefficients in [-1, 1]: the walls x=0, x=Lx, y=0, y=Ly, z=0, z=Lz
%   sourcePos       [Q x 3], each row strictly inside the room; arrayPos [x y z] inside the room
%   maxDelay        samples: components that arrive later are left out
%   maxOrder        ([]: no limit) the largest reflection order kept
%   sources         cell of Q arrays [J_q x 4] with the columns azimuth, zenith, delay in samples and gain (1/distance times the
%                   walls' coefficients; a unit source at 1 m in the free field has gain 1), in the definition's order: the
%                   `sources` of getArrayIrs
%   distances       (second output, on request) cell of Q arrays [J_q x 1], the components' distances in metres: the 'distance' of
%                   getArrayIrs (DESIGN.md section 14)
%   emission        (third output, on request) cell of Q arrays [J_q x 3]: the unit vectors in room axes along which the components'
%                   rays left the real source, the 'emission' of getArrayIrs (DESIGN.md section 15)
p = struct('maxOrder', []);
for i = 1:2:numel(varargin)
    if ~isfield(p, varargin{i}); error('eMagLS:arg', 'unknown option "%s"', varargin{i}); end
    p.(varargin{i}) = varargin{i + 1};
end
if size(sourcePos, 2) ~= 3; error('eMagLS:arg', 'sourcePos must be [Q x 3]'); end
args = {'shoebox_components', double(roomDim(:)), double(wallReflection(:)), double(sourcePos), double(arrayPos(:)), double(fs), ...
    double(maxDelay), double(p.maxOrder)};
if nargout > 2
    [compPtr, comps, dists, emit] = emagls_mex(args{:});
elseif nargout > 1
    [compPtr, comps, dists] = emagls_mex(args{:});
else
    [compPtr, comps] = emagls_mex(args{:});
end
Q = size(sourcePos, 1);
sources = cell(Q, 1);
distances = cell(Q, 1);
emission = cell(Q, 1);
for q = 1:Q
    sources{q} = comps(compPtr(q) + 1:compPtr(q + 1), :);
    if nargout > 1; distances{q} = dists(compPtr(q) + 1:compPtr(q + 1)); end
    if nargout > 2; emission{q} = emit(compPtr(q) + 1:compPtr(q + 1), :); end
end
end
