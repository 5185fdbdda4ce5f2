function [irs, counts] = getArrayRoomIrs(roomDim, wallReflection, sourcePos, arrayPos, fs, irLen, preDelay, micRadius, micGridAziZenRad, varargin)
% Impulse responses of the simulated rigid-sphere array in a shoebox room, on the MI355X library (DESIGN.md section 12;
% include/emagls.h, emagls_array_room_irs): getArrayIrs(getShoeboxComponents(...), ...) bit for bit, with the image sources
% enumerated on the device and fed to the responses' kernels there.
%   [irs, counts] = getArrayRoomIrs(roomDim, wallReflection, sourcePos, arrayPos, fs, irLen, preDelay, micRadius, micGridAziZenRad, ...
%                                   'name', value, ...)
%   the room as in getShoeboxComponents (the array's whole sphere inside it, every source outside the sphere), the array as in
%   getArrayIrs; further names: order (4), encoder ([]), nfft ([]) as there, maxOrder ([]: no limit on the reflection order),
%   maxDelay ([]: irLen - 1 - preDelay samples; maxDelay + preDelay beyond nfft - 1 would wrap and is refused)
%   the spectral room (DESIGN.md section 13; emagls_array_room_irs_spectral): wallReflection [6 x P], one reflection spectrum per wall
%   over the P = nfft/2 + 1 bins, and / or the name airAttenuation ([]), [P] in Np/m, each component's path its distance (six
%   coefficients with it are repeated over the bins); then every image within maxOrder and maxDelay is a component
%   waveModel ('planeWave', getSMAIRMatrix's parameter and default): 'pointSource' makes every image a point source at its distance
%   (DESIGN.md section 14; emagls_array_room_irs_point): getArrayIrs with 'distance' on the lists of getShoeboxComponents, bit for bit
%   directive sources (DESIGN.md section 15; emagls_array_room_irs_directive): directivity ([]) and sourceOrientation ([]) as in
%   getArrayIrs, with every wall and wave model above; the emission vectors are the enumeration's, and the result is getArrayIrs on
%   the lists and emission vectors of getShoeboxComponents / getShoeboxImages, bit for bit
%   irs       [irLen x numChannels x Q] (complex with a complex encoder): irs(:, :, q) is the rir of sourceFieldStream
%   counts    [Q x 1] the number of image sources of each source position
p = struct('order', 4, 'encoder', [], 'nfft', [], 'maxOrder', [], 'maxDelay', [], 'airAttenuation', [], 'waveModel', 'planeWave', ...
    'sourceOrientation', [], 'directivity', []);
for i = 1:2:numel(varargin)
    if ~isfield(p, varargin{i}); error('eMagLS:arg', 'unknown option "%s"', varargin{i}); end
    p.(varargin{i}) = varargin{i + 1};
end
if size(sourcePos, 2) ~= 3; error('eMagLS:arg', 'sourcePos must be [Q x 3]'); end
if numel(wallReflection) == 6; wallReflection = wallReflection(:); end
rot = [];
coef = [];
if isempty(p.directivity) && ~isempty(p.sourceOrientation); error('eMagLS:arg', 'sourceOrientation comes with a directivity'); end
if ~isempty(p.directivity)
    nfft = double(p.nfft);
    if isempty(nfft); nfft = min(65536, max(8, 2^nextpow2(2 * double(irLen)))); end
    [rot, coef] = emaglsDirectiveArgs(p.sourceOrientation, p.directivity, size(sourcePos, 1), nfft / 2 + 1);
end
[irs, counts] = emagls_mex('array_room_irs', double(roomDim(:)), double(wallReflection), double(sourcePos), double(arrayPos(:)), double(fs), ...
    double(irLen), double(preDelay), double(micRadius), double(micGridAziZenRad), double(p.order), double(p.encoder), double(p.nfft), ...
    double(p.maxOrder), double(p.maxDelay), double(p.airAttenuation(:)), char(p.waveModel), rot, coef);
end
